"""NumPy restatement of the reference's ChordsFeature (features/chords.cpp:11-111): MAXCHORDS_* and ALLCHORDS_*, on
Rotation::rotate_cloud (rotation.cpp:70-91), ImageMatrix(cloud) (image_matrix.h:256-277), ImageMatrix::get_chlen
(image_matrix.cpp:206-237), Moments2 (moments.h:10-45) and TrivialHistogram (histogram.h:115-119, :268-309).

Same operation order, float32 casts where the reference has `float`, Python floats (IEEE doubles) everywhere else, and the
platform libm for sin / cos -- what the reference and the host side of the HIP path call.  What is restated, quirks included:
  * the angles are the partial sums of `ang += M_PI / 20` (20 of them); sin / cos take the angle rounded to float;
  * a rotated coordinate is rounded to float and then truncated TOWARD ZERO;
  * the dense plane is assigned in cloud order: where several pixels land on one cell the last one decides, and a cell is signal
    iff that pixel's intensity is non-zero;
  * a column's chord is its longest run of signal cells that a zero cell closes: a run that reaches the last row does not count;
  * one TrivialHistogram serves both closings and initialize_uniques() appends: ALLCHORDS_MODE and ALLCHORDS_MEDIAN are taken
    over the max chords FOLLOWED BY all chords (every per-angle maximum counts twice).
tests/test_chords_cpu.py pins this file to the recorded output of the reference class; the GPU tests and tools/chords_fuzz.py use
it where no recording exists."""
from __future__ import annotations

import math

import numpy as np

N_ANGLES = 20
N_SIDE = 100
_ST = ("MAX", "MAX_ANG", "MIN", "MIN_ANG", "MEDIAN", "MEAN", "MODE", "STDDEV")
NAMES = ["MAXCHORDS_" + k for k in _ST] + ["ALLCHORDS_" + k for k in _ST]
APPROX = ("MAXCHORDS_MEAN", "MAXCHORDS_STDDEV", "ALLCHORDS_MEAN", "ALLCHORDS_STDDEV")   # every other column is compared exactly


def angles():
    """The loop `for (double ang = 0; ang < M_PI; ang += M_PI / 20.0)` itself."""
    out = []
    step = math.pi / float(N_ANGLES)
    ang = 0.0
    while ang < math.pi:
        out.append(ang)
        ang += step
    return out


def sincos_table():
    """(sin, cos) per angle as rotate_cloud computes them: the angle passed as float, sin / cos of its double value."""
    return [(math.sin(float(np.float32(a))), math.cos(float(np.float32(a)))) for a in angles()]


def rotated_cells(x, y, ox, oy, w, h, s, c):
    """Integer cell coordinates (xi, yi) of the absolute cloud turned about the centre of its box."""
    xmin, ymin = int(ox), int(oy)
    cx = float(xmin + (xmin + int(w) - 1)) / 2.0
    cy = float(ymin + (ymin + int(h) - 1)) / 2.0
    px = (np.asarray(x, np.int64) + xmin).astype(np.float64)
    py = (np.asarray(y, np.int64) + ymin).astype(np.float64)
    xr = ((px - cx) * c - (py - cy) * s) + cx
    yr = ((py - cy) * c + (px - cx) * s) + cy
    xi = np.trunc(xr.astype(np.float32)).astype(np.int64)
    yi = np.trunc(yr.astype(np.float32)).astype(np.int64)
    return xi, yi


def column_chords(xi, yi, inten):
    """Chord lengths (zeros included) of the selected columns of the dense plane of one rotated cloud, and the plane's width."""
    x0, y0 = int(xi.min()), int(yi.min())
    W, H = int(xi.max()) - x0 + 1, int(yi.max()) - y0 + 1
    cell = (yi - y0) * W + (xi - x0)
    last = np.full(W * H, -1, np.int64)
    np.maximum.at(last, cell, np.arange(len(cell), dtype=np.int64))          # the last pixel of the cloud on every cell
    sig = np.zeros(W * H, bool)
    hit = last >= 0
    sig[hit] = np.asarray(inten)[last[hit]] != 0
    step = W // N_SIDE if W >= 2 * N_SIDE else 1
    cols = np.arange(0, W, step)
    V = sig.reshape(H, W)[:, cols].T                                         # (columns, rows)
    F = np.zeros((len(cols), H + 2), np.int8)
    F[:, 1:H + 1] = V
    d = np.diff(F.ravel())
    st = np.nonzero(d == 1)[0] + 1                                           # first cell of every run, first cell behind it
    en = np.nonzero(d == -1)[0] + 1
    closed = (en % (H + 2)) != H + 1                                         # the closing cell is a cell of the plane
    ch = np.zeros(len(cols), np.int64)
    np.maximum.at(ch, (st // (H + 2))[closed], (en - st)[closed])
    return ch, W


def per_angle(x, y, inten, ox, oy, w, h, tab=None):
    """[chords > 0 in column order] per angle."""
    tab = tab or sincos_table()
    out = []
    for s, c in tab:
        xi, yi = rotated_cells(x, y, ox, oy, w, h, s, c)
        ch, _ = column_chords(xi, yi, inten)
        out.append([int(v) for v in ch if v > 0])
    return out


def _moments2(D):
    n, mean, m2 = 0, 0.0, 0.0
    for v in D:
        x = float(v)
        n1 = n
        n += 1
        delta = x - mean
        delta_n = delta / n
        term1 = delta * delta_n * n1
        mean = mean + delta_n
        m2 += term1
    return mean, (math.sqrt(m2 / (n - 1)) if n > 2 else 0.0)


def _mode_median(U):
    vals, cnt = np.unique(np.asarray(U, np.int64), return_counts=True)
    mode = int(vals[np.argmax(cnt)])                                         # the smallest among the most frequent
    S = sorted(U)
    n = len(S)
    med = float(S[n // 2]) if n % 2 else float(S[n // 2] + S[n // 2 - 1]) / 2.0
    return float(mode), med


def close(chords, ang=None):
    """The 16 columns (NAMES order) from the per-angle chord lists."""
    ang = ang or angles()
    MC, MA, AC, AA = [], [], [], []
    for k, T in enumerate(chords):
        for v in T:
            AC.append(v)
            AA.append(ang[k])
        if T:
            MC.append(max(T))
            MA.append(ang[k])
    if not MC:
        return [0.0] * 16
    out = []
    U = []
    for D, A in ((MC, MA), (AC, AA)):
        U = U + D                                                            # (initialize_uniques appends)
        mean, sd = _moments2(D)
        mode, med = _mode_median(U)
        out += [float(max(D)), A[D.index(max(D))], float(min(D)), A[D.index(min(D))], med, mean, mode, sd]
    return out


def row(x, y, inten, ox, oy, w, h, tab=None):
    return close(per_angle(x, y, inten, ox, oy, w, h, tab))


def _origins(b, origin):
    if origin is not None:
        return origin
    if getattr(b, "origin_x", None) is not None:
        return b.origin_x, b.origin_y
    z = np.zeros(b.n_roi, np.int64)
    return z, z


def batch_per_angle(b, origin=None):
    tab = sincos_table()
    ox, oy = _origins(b, origin)
    off = b.px_offset.astype(np.int64)
    return [per_angle(b.x[off[r]:off[r + 1]], b.y[off[r]:off[r + 1]], b.inten[off[r]:off[r + 1]], ox[r], oy[r], b.bbox_w[r], b.bbox_h[r], tab)
            for r in range(b.n_roi)]


def table(b, origin=None):
    """(n_roi, 16) for a HostBatch; origin = (origin_x, origin_y) arrays, the batch's own when it has them, else zeros."""
    ang = angles()
    return np.array([close(P, ang) for P in batch_per_angle(b, origin)], np.float64).reshape(b.n_roi, 16)


def summary(P):
    """(per-angle maximum, count, sum) arrays [20] of one ROI's chord lists -- what the fixtures record per angle."""
    return (np.array([max(T) if T else 0 for T in P], np.int64), np.array([len(T) for T in P], np.int64),
            np.array([sum(T) for T in P], np.int64))


def libm_sensitive(b, origin=None):
    """ROIs of which a pixel changes its cell when every sin / cos of the table moves by one unit in the last place, in any of the
    four sign combinations: fixtures on which a last-bit difference of the host libm could change a chord."""
    base = sincos_table()
    ox, oy = _origins(b, origin)
    off = b.px_offset.astype(np.int64)
    bad = []
    for r in range(b.n_roi):
        x, y = b.x[off[r]:off[r + 1]], b.y[off[r]:off[r + 1]]
        hit = False
        for sv, cv in base:
            xi, yi = rotated_cells(x, y, ox[r], oy[r], b.bbox_w[r], b.bbox_h[r], sv, cv)
            for ds in (-math.inf, math.inf):
                for dc in (-math.inf, math.inf):
                    xj, yj = rotated_cells(x, y, ox[r], oy[r], b.bbox_w[r], b.bbox_h[r], math.nextafter(sv, ds), math.nextafter(cv, dc))
                    hit = hit or bool((xi != xj).any() or (yi != yj).any())
        if hit:
            bad.append(r)
    return bad
