"""numpy restatement of two classes of the reference's shape block, as the HIP path serves them (nyxus_amd/csrc/roi_circle.hip):

    EnclosingInscribingCircumscribingCircleFeature  features/circle.cpp:28-244 (centroid: basic_morphology.cpp:40-47)
    GeodeticLengthThicknessFeature                  features/geo_len_thickness.cpp:22-35 (perimeter: contour.cpp:960-974)

Takes a HostBatch plus the ROIs' merged contours (padded coordinates, walk order; without `contours` they come from the C oracle's
`nyxo_contour`, see tests/radial_ref.py).  The reference's Pixel2 is `padded + origin` in integers (contour.cpp:673-679).

Every decision of the minimum enclosing circle is a float comparison, so the restatement makes the reference's float operations one
by one in numpy's float32 (never fused; numpy's float32 division and square root are correctly rounded).  The three nested scans are
written as "first point that fails the test, one update, go on behind it": the per-point test has no state but centre and radius,
so this is the reference's loop.  The quirks are the reference's: Pixel2::operator/ and operator* truncate to integers, normL2 is a
square root that findCircle3pts roots again, the unqualified sqrt of circle.cpp:63 is the double one (so `* 0.5f + EPS` is added in
double and rounded once), EPS = 1e-4f.  tests/test_circle_cpu.py pins this module bit for bit to values recorded from the classes."""
from __future__ import annotations

import math

import numpy as np

CIRCLES = ["DIAMETER_MIN_ENCLOSING_CIRCLE", "DIAMETER_CIRCUMSCRIBING_CIRCLE", "DIAMETER_INSCRIBING_CIRCLE"]
GEODETIC = ["GEODETIC_LENGTH", "THICKNESS"]
NAMES = CIRCLES + GEODETIC
EXTRA = ["PERIMETER", "CENTROID_X", "CENTROID_Y"]          # recorded beside the five columns; not columns of the HIP path

F = np.float32
EPS = F(1.0e-4)
TWO, HALF = F(2.0), F(0.5)
CHUNK = 256


def _norm(dx, dy):
    """Point2f::normL2 (pixel.h:23)."""
    return np.sqrt(dx * dx + dy * dy)


def _first_out(PX, PY, lo, hi, cx, cy, r):
    """First index in [lo, hi) whose point is not strictly inside the circle, or hi."""
    while lo < hi:
        e = min(hi, lo + CHUNK)
        dx, dy = cx - PX[lo:e], cy - PY[lo:e]
        out = ~(_norm(dx, dy) < r)
        k = int(np.argmax(out))
        if out[k]:
            return lo + k
        lo = e
    return hi


def _trunc_div2(v):
    """Pixel2::operator/ (2.0f), then operator Point2f: (float) StatsInt((float) v / 2.0f)."""
    return F(int(F(v) / TWO))


def _trunc_half(v):
    """Pixel2::operator* (0.5f), then operator Point2f."""
    return F(int(F(v) * HALF))


def circle3(p0, p1, p2):
    """findCircle3pts (circle.cpp:42-85); points are (x, y) Python integers."""
    v1x, v1y = F(p1[0] - p0[0]), F(p1[1] - p0[1])
    v2x, v2y = F(p2[0] - p0[0]), F(p2[1] - p0[1])
    m1x, m1y = _trunc_div2(p0[0] + p1[0]), _trunc_div2(p0[1] + p1[1])
    c1 = m1x * v1x + m1y * v1y
    m2x, m2y = _trunc_div2(p0[0] + p2[0]), _trunc_div2(p0[1] + p2[1])
    c2 = m2x * v2x + m2y * v2y
    det = v1x * v2y - v1y * v2x
    if abs(det) <= EPS:
        d1 = _norm(F(p0[0] - p1[0]), F(p0[1] - p1[1]))
        d2 = _norm(F(p0[0] - p2[0]), F(p0[1] - p2[1]))
        d3 = _norm(F(p1[0] - p2[0]), F(p1[1] - p2[1]))
        radius = F(math.sqrt(float(max(d1, d2, d3))) * 0.5 + float(EPS))     # sqrt(double) * 0.5f + EPS in double, one rounding
        if d1 >= d2 and d1 >= d3:
            a, b = p0, p1
        elif d2 >= d1 and d2 >= d3:
            a, b = p0, p2
        else:
            a, b = p1, p2
        return _trunc_half(a[0] + b[0]), _trunc_half(a[1] + b[1]), radius
    cx = (c1 * v2y - c2 * v1y) / det
    cy = (v1x * c2 - v2x * c1) / det
    ex, ey = cx - F(p0[0]), cy - F(p0[1])
    return cx, cy, np.sqrt(ex * ex + ey * ey) + EPS


def _two_point(X, Y, a, b):
    cx, cy = F(int(X[a] + X[b])) / TWO, F(int(Y[a] + Y[b])) / TWO
    r = _norm(F(int(X[a] - X[b])), F(int(Y[a] - Y[b]))) / TWO + EPS
    return cx, cy, r


def min_enclosing_radius(X, Y, stats=None):
    """minEnclosingCircle (circle.cpp:145-217) over absolute integer coordinates X, Y (int64 arrays): the float radius."""
    n = len(X)
    if n == 0:
        return F(0)
    if n == 1:
        return EPS
    PX, PY = X.astype(F), Y.astype(F)
    if n == 2:
        return F(float(_norm(PX[0] - PX[1], PY[0] - PY[1])) / 2.0) + EPS
    steps = 0
    cx, cy, r = _two_point(X, Y, 0, 1)
    i = 2
    while True:
        i = _first_out(PX, PY, i, n, cx, cy, r)                              # (dx = p - c there, c - p here: the squares are the same)
        if i >= n:
            break
        # findSecondPoint
        c2x, c2y, r2 = _two_point(X, Y, 0, i)
        j = 1
        while True:
            j = _first_out(PX, PY, j, i, c2x, c2y, r2)
            if j >= i:
                break
            # findThirdPoint
            c3x, c3y, r3 = _two_point(X, Y, j, i)
            k = 0
            while True:
                k = _first_out(PX, PY, k, j, c3x, c3y, r3)
                if k >= j:
                    break
                nx, ny, nr = circle3((int(X[i]), int(Y[i])), (int(X[j]), int(Y[j])), (int(X[k]), int(Y[k])))
                steps += 1
                if nr > 0:
                    c3x, c3y, r3 = nx, ny, nr
                k += 1
            if r3 > 0:
                c2x, c2y, r2 = c3x, c3y, r3
            j += 1
        if r2 > 0:
            cx, cy, r = c2x, c2y, r2
        i += 1
    if stats is not None:
        stats["circle3"] = steps
    return r


def roi_row(x, y, K, ox, oy):
    """(the five columns, PERIMETER, CENTROID_X, CENTROID_Y, clamped) of one ROI: x, y box-relative cloud, K (nK, 2) padded contour,
    (ox, oy) the box origin.  `clamped`: SqRootTmp < 0 was taken."""
    n = len(x)
    row = np.zeros(8)
    if n == 0:
        return row, False
    sx = int(np.asarray(x, np.int64).sum()) + n * int(ox)
    sy = int(np.asarray(y, np.int64).sum()) + n * int(oy)
    cx, cy = float(sx) / float(n), float(sy) / float(n)
    row[6], row[7] = cx, cy
    nK = len(K)
    X = np.asarray(K[:, 0], np.int64) + int(ox) if nK else np.zeros(0, np.int64)
    Y = np.asarray(K[:, 1], np.int64) + int(oy) if nK else np.zeros(0, np.int64)
    per = 0.0
    if nK:
        row[0] = 2.0 * float(min_enclosing_radius(X, Y))
        tx, ty = X.astype(np.float64) - (cx - 1.0), Y.astype(np.float64) - (cy - 1.0)
        d = np.sqrt(tx * tx + ty * ty)
        row[1], row[2] = 2.0 * d.max(), 2.0 * d.min()
        dx, dy = X - np.roll(X, 1), Y - np.roll(Y, 1)                        # term 0: the last point to the first
        for t in np.sqrt((dx * dx + dy * dy).astype(np.float64)):
            per += float(t)                                                  # the reference's order
    row[5] = per
    sq = per * per / 16.0 - float(n)
    clamped = sq < 0
    if clamped:
        sq = 0.0
    row[3] = per / 4.0 + math.sqrt(sq)
    row[4] = per / 2.0 - row[3]
    return row, bool(clamped)


def table(b, contours=None, with_flags=False):
    """(n_roi, 8): the five columns, then PERIMETER, CENTROID_X, CENTROID_Y."""
    if contours is None:
        from tests.radial_ref import contours_of
        contours = contours_of(b)
    T = np.zeros((b.n_roi, 8))
    flags = np.zeros(b.n_roi, bool)
    for r in range(b.n_roi):
        o, e = int(b.px_offset[r]), int(b.px_offset[r + 1])
        ox = int(b.origin_x[r]) if b.origin_x is not None else 0
        oy = int(b.origin_y[r]) if b.origin_y is not None else 0
        T[r], flags[r] = roi_row(b.x[o:e], b.y[o:e], contours[r], ox, oy)
    return (T, flags) if with_flags else T
