"""NumPy restatement of the reference's three caliper classes (features/caliper_feret.cpp, caliper_martin.cpp,
caliper_nassenstein.cpp) on the convex hull of ConvexHullFeature::build_convex_hull (convex_hull_nontriv.cpp:68-120), rotated by
Rotation::rotate_around_center_fp (rotation.cpp:37-68) and closed by ComputeCommonStatistics2 (common_stats.cpp:9-72).

Same operation order, float32 casts where the reference has `float`, Python floats (IEEE doubles) everywhere else, and the
platform libm for sin / cos -- what the reference and the host side of the HIP path call.  tests/test_caliper_cpu.py pins this
file to the recorded output of the reference classes; the GPU tests and tools/caliper_fuzz.py use it where no recording exists."""
from __future__ import annotations

import math

import numpy as np

N_FERET_ANGLES = 19          # theta = 0, 10, ..., 180 (theta <= 180)
N_ANGLES = 18                # theta = 0, 10, ..., 170 (theta < 180): Martin, Nassenstein
N_GRID = 100                 # Martin: midpoint levels per angle
NAMES = (["MIN_FERET_ANGLE", "MAX_FERET_ANGLE"] + ["STAT_FERET_DIAM_" + k for k in ("MIN", "MAX", "MEAN", "MEDIAN", "STDDEV", "MODE")]
         + ["STAT_MARTIN_DIAM_" + k for k in ("MIN", "MAX", "MEAN", "MEDIAN", "STDDEV", "MODE")]
         + ["STAT_NASSENSTEIN_DIAM_" + k for k in ("MIN", "MAX", "MEAN", "MEDIAN", "STDDEV", "MODE")])
EXACT = ("MIN_FERET_ANGLE", "MAX_FERET_ANGLE", "STAT_FERET_DIAM_MODE", "STAT_MARTIN_DIAM_MODE", "STAT_NASSENSTEIN_DIAM_MODE")


def sincos_table():
    """(sin, cos) per angle 0, 10, ..., 180 as rotation.cpp computes them: the angle in float, sin / cos of its double value."""
    out = []
    for k in range(N_FERET_ANGLES):
        t = np.float32(np.float32(np.float32(10 * k) * np.float32(math.pi)) / np.float32(180.0))
        out.append((math.sin(float(t)), math.cos(float(t))))
    return out


def _right_turn(p1, p2, p3):
    return (p3[0] - p1[0]) * (p2[1] - p1[1]) - (p3[1] - p1[1]) * (p2[0] - p1[0]) > 0


def _chain(pts):
    """Monotone chain over points in (x, y) order: the upper chain, then the lower chain's points that are not present yet."""
    n = len(pts)
    if n < 2:
        return []
    up = [pts[0], pts[1]]
    for i in range(2, n):
        while len(up) > 1 and not _right_turn(up[-2], up[-1], pts[i]):
            up.pop()
        up.append(pts[i])
    lo = [pts[n - 1], pts[n - 2]]
    for i in range(2, n):
        while len(lo) > 1 and not _right_turn(lo[-2], lo[-1], pts[n - i - 1]):
            lo.pop()
        lo.append(pts[n - i - 1])
    for p in lo:
        if p not in up:
            up.append(p)
    return up


def hull_all_pixels(x, y):
    """build_convex_hull over every pixel of the ROI (n < 2: empty)."""
    pts = sorted(set(zip((int(v) for v in x), (int(v) for v in y))))
    if len(x) < 2:
        return []
    return _chain(pts)


def column_extremes(x, y):
    """The lowest and the highest pixel of every occupied column, in (x, y) order (one point where they coincide)."""
    x = np.asarray(x, np.int64); y = np.asarray(y, np.int64)
    x0 = int(x.min())
    w = int(x.max()) - x0 + 1
    lo = np.full(w, np.iinfo(np.int64).max); hi = np.full(w, np.iinfo(np.int64).min)
    np.minimum.at(lo, x - x0, y)
    np.maximum.at(hi, x - x0, y)
    pts = []
    for c in range(w):
        if hi[c] < lo[c]:
            continue
        pts.append((c + x0, int(lo[c])))
        if hi[c] != lo[c]:
            pts.append((c + x0, int(hi[c])))
    return pts


def hull(x, y):
    """The hull as the HIP kernel builds it: the chain over the per-column extremes."""
    if len(x) < 2:
        return []
    return _chain(column_extremes(x, y))


def rotate(H, s, c):
    """rotate_around_center_fp: float32 vertices of the hull turned about the mean of its vertices."""
    n = len(H)
    cx = float(sum(p[0] for p in H)) / float(n)
    cy = float(sum(p[1] for p in H)) / float(n)
    out = []
    for px, py in H:
        x_rot = (px - cx) * c - (py - cy) * s + cx
        y_rot = (py - cy) * c + (px - cx) * s + cy
        out.append((float(np.float32(x_rot)), float(np.float32(y_rot))))
    return out


def _span_at(P, v, axis):
    """hull_width_at_y (axis = 1: cut y = v, x extent) / hull_height_at_x (axis = 0: cut x = v, y extent)."""
    o = 1 - axis
    have = False
    lo = hi = 0.0
    n = len(P)
    for i in range(n):
        a, b = P[i], P[(i + 1) % n]
        ac, bc = a[axis], b[axis]
        if v < min(ac, bc) or v > max(ac, bc):
            continue
        if bc != ac:
            d = float(np.float32(b[o]) - np.float32(a[o]))          # float operands: a float difference
            e0 = e1 = a[o] + d * (v - ac) / (bc - ac)
        else:
            e0, e1 = min(a[o], b[o]), max(a[o], b[o])
        if not have:
            lo, hi, have = e0, e1, True
        else:
            lo, hi = min(lo, e0), max(hi, e1)
    return hi - lo if have else 0.0


def feret_list(H, tab):
    """[(angle, diameter)] of the angles whose diameter is > 0."""
    out = []
    for k in range(N_FERET_ANGLES):
        P = rotate(H, *tab[k])
        xs = [p[0] for p in P]
        d = max(xs) - min(xs)
        if d > 0:
            out.append((float(10 * k), d))
    return out


def martin_list(H, tab):
    out = []
    for k in range(N_ANGLES):
        P = rotate(H, *tab[k])
        ys = [p[1] for p in P]
        mn, mx = min(ys), max(ys)
        if mx <= mn:
            continue
        step = (mx - mn) / N_GRID
        w = [_span_at(P, mn + (i + 0.5) * step, 1) for i in range(N_GRID)]
        total = 0.0
        for v in w:
            total += v
        if total <= 0.0:
            continue
        half, cum, m = 0.5 * total, 0.0, w[-1]
        for v in w:
            cum += v
            if cum >= half:
                m = v
                break
        out.append(m)
    return out


def nassenstein_list(H, tab):
    out = []
    if len(H) < 3:
        return out
    for k in range(N_ANGLES):
        P = rotate(H, *tab[k])
        ymax = max(p[1] for p in P)
        xsum, cnt = 0.0, 0
        for p in P:
            if abs(p[1] - ymax) < 1e-3:
                xsum += p[0]
                cnt += 1
        out.append(_span_at(P, xsum / max(cnt, 1), 0))
    return out


def stats(D):
    """ComputeCommonStatistics2: min, max, mean, median, stddev (divisor n), mode (truncation histogram, first maximum bin)."""
    if not D:
        return [0.0] * 6
    n = len(D)
    mx, mn = max(D), min(D)
    s = 0.0
    for v in D:
        s += v
    mean = s / n
    ss = 0.0
    for v in D:
        ss += (v - mean) * (v - mean)
    sd = math.sqrt(ss / n)
    imin = int(math.floor(mn))
    bins = [0] * (int(math.ceil(mx)) - imin + 1)
    for v in D:
        bins[int(v) - imin] += 1
    best, best_i = 0, -1
    for i, c in enumerate(bins):
        if c > best:
            best, best_i = c, i
    S = sorted(D)
    med = (S[n // 2] + S[n // 2 - 1]) / 2.0 if n % 2 == 0 else S[n // 2]
    return [mn, mx, mean, med, sd, float(best_i + imin)]


def diameters(x, y, ox=0, oy=0, tab=None, H=None):
    """(feret [(angle, d)], martin [d], nassenstein [d]) of one ROI with relative pixels x, y and box origin (ox, oy)."""
    tab = tab or sincos_table()
    if H is None:
        H = hull(x, y)
    if not H:
        return [], [], []
    H = [(px + int(ox), py + int(oy)) for px, py in H]
    return feret_list(H, tab), martin_list(H, tab), nassenstein_list(H, tab)


def row(x, y, ox=0, oy=0, soft_nan=0.0, tab=None):
    """The 20 columns of one ROI, NAMES order."""
    H = hull(x, y)
    if not H:
        return [soft_nan] * 20
    F, M, N = diameters(x, y, ox, oy, tab, H)
    if F:
        d = [v for _, v in F]
        i_min = min(range(len(d)), key=lambda i: (d[i], i))          # the first minimum / the first maximum (get_minmax_idx)
        i_max = max(range(len(d)), key=lambda i: (d[i], -i))
        fr = [F[i_min][0], F[i_max][0]] + stats(d)
    else:
        fr = [soft_nan] * 8
    return fr + stats(M) + stats(N)


def table(b, origin=None, soft_nan=0.0):
    """(n_roi, 20) for a HostBatch; origin = (origin_x, origin_y) arrays, the batch's own when it has them, else zeros."""
    tab = sincos_table()
    ox, oy = _origins(b, origin)
    off = b.px_offset.astype(np.int64)
    return np.array([row(b.x[off[r]:off[r + 1]], b.y[off[r]:off[r + 1]], ox[r], oy[r], soft_nan, tab) for r in range(b.n_roi)], np.float64).reshape(b.n_roi, 20)


def _origins(b, origin):
    if origin is not None:
        return origin
    if getattr(b, "origin_x", None) is not None:
        return b.origin_x, b.origin_y
    z = np.zeros(b.n_roi, np.int64)
    return z, z


def near_integer(b, origin=None, eps=1e-4):
    """ROIs with a per-angle diameter within eps of an integer without being that integer.  (Every lattice shape has such values at
    90 and 180 degrees: the reference's angle is a float, so cos(90 deg) = -4.4e-8 and an integer extent comes out as 2.0000002.)"""
    tab = sincos_table()
    bad = []
    ox, oy = _origins(b, origin)
    off = b.px_offset.astype(np.int64)
    for r in range(b.n_roi):
        F, M, N = diameters(b.x[off[r]:off[r + 1]], b.y[off[r]:off[r + 1]], ox[r], oy[r], tab)
        for v in [d for _, d in F] + M + N:
            k = round(v)
            if v != k and abs(v - k) < eps:
                bad.append(r)
                break
    return bad


def libm_sensitive(b, origin=None):
    """ROIs whose integer-valued columns (the two angles, the three modes) change when every sin / cos of the table moves by one
    unit in the last place, in any of the four sign combinations: fixtures on which a last-bit difference of the host libm could
    flip a mode."""
    base = sincos_table()
    ox, oy = _origins(b, origin)
    off = b.px_offset.astype(np.int64)
    idx = [NAMES.index(n) for n in EXACT]
    bad = []
    for r in range(b.n_roi):
        x, y = b.x[off[r]:off[r + 1]], b.y[off[r]:off[r + 1]]
        want = [row(x, y, ox[r], oy[r], 0.0, base)[i] for i in idx]
        for ds in (-math.inf, math.inf):
            for dc in (-math.inf, math.inf):
                tab = [(math.nextafter(sv, ds), math.nextafter(cv, dc)) for sv, cv in base]
                if [row(x, y, ox[r], oy[r], 0.0, tab)[i] for i in idx] != want:
                    bad.append(r)
                    break
            else:
                continue
            break
    return bad
