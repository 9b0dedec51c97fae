"""NumPy restatement of the reference's FractalDimensionFeature, EulerNumberFeature (mode 8) and RoiRadiusFeature: own code,
written from the reference's features/fractal_dim.cpp:20-99, :127-191, euler_number.cpp:44-103 and roi_radius.cpp:11-37.

Takes a HostBatch plus the ROIs' merged contours (padded coordinates, walk order; tests/radial_ref.py contours_of by default).
tests/test_outline_cpu.py pins this module to tables recorded from the reference classes (tests/golden/outline); it then serves
arbitrary inputs: fuzz, mixed masks, pixel-order permutations.
"""
from __future__ import annotations

import math

import numpy as np

from tests.radial_ref import contours_of, min_sqdist

NAMES = ["FRACT_DIM_BOXCOUNT", "FRACT_DIM_PERIMETER", "EULER_NUMBER", "ROI_RADIUS_MEAN", "ROI_RADIUS_MAX", "ROI_RADIUS_MEDIAN"]


def ceil_pow2(a):
    return 1 if a <= 1 else 1 << (int(a) - 1).bit_length()


def loglog_slope(points):
    """fractal_dim.cpp:169-191, the summation order as written."""
    sx = sy = sxy = sx2 = 0.0
    used = 0
    for px, py in points:
        if px <= 0.0 or py <= 0.0:
            continue
        lx, ly = math.log(px), math.log(py)
        sx += lx
        sy += ly
        sxy += lx * ly
        sx2 += lx * lx
        used += 1
    if used < 2:
        return 0.0
    denom = sx2 * float(used) - sx * sx
    if denom == 0.0:
        return 0.0
    return (sxy * float(used) - sx * sy) / denom


def box_counts(x, y, w, h):
    """[(box size, [counts per grid origin])] for box sizes padded side .. 2: four origins when the padded side is <= 32, else one."""
    side = ceil_pow2(max(w, h))
    out = []
    s = side
    while s > 1:
        origins = [(0, 0), (s // 2, 0), (0, s // 2), (s // 2, s // 2)] if side <= 32 else [(0, 0)]
        out.append((s, [len(np.unique(((y + oy) // s) * 65536 + (x + ox) // s)) for ox, oy in origins]))
        s //= 2
    return out


def boxcount_fd(x, y, w, h):
    if len(x) < 2:
        return 0.0
    return -loglog_slope([(float(s), float(min(c))) for s, c in box_counts(x, y, w, h)])


def perimeter_fd(K):
    n = len(K)
    if n < 3:
        return 0.0
    pts = []
    s = n // 4
    while s > 0:
        perim, nsteps, i = 0.0, 0, 0
        while i + s < n:
            d = K[i] - K[i + s]
            perim += math.sqrt(float(d[0] * d[0] + d[1] * d[1]))
            nsteps += 1
            i += s
        d = K[i] - K[0]
        perim += math.sqrt(float(d[0] * d[0] + d[1] * d[1]))
        nsteps += 1
        pts.append((perim / float(nsteps), perim))
        s //= 2
    return 1.0 - loglog_slope(pts)


def euler_number(x, y, w, h):
    """Mode 8: quads of the padded plane (euler_number.cpp:60-102), integer division truncating toward zero."""
    p = np.zeros((h + 2, w + 2), np.int64)
    p[y + 1, x + 1] = 1
    q = 8 * p[:-1, :-1] + 4 * p[:-1, 1:] + 2 * p[1:, :-1] + p[1:, 1:]
    c1 = int(np.isin(q, (8, 4, 2, 1)).sum())
    c3 = int(np.isin(q, (7, 11, 13, 14)).sum())
    cd = int(np.isin(q, (9, 6)).sum())
    v = c1 - c3 - 2 * cd
    return float(-((-v) // 4) if v < 0 else v // 4)


def roi_radius(x, y, K):
    """(mean, max, median) of the integer squared distances to the contour; None where the reference is undefined (a one-point
    contour: the first step of the hill descent converts 1 / log(1) to int)."""
    if len(K) == 1:
        return None
    if len(K) == 0:
        return 0.0, 0.0, 0.0
    d = np.array([min_sqdist(int(a), int(b), K) for a, b in zip(x, y)], np.int64)
    s = np.sort(d)
    n = len(s)
    med = float(s[n // 2]) if n % 2 else float(int(s[n // 2]) + int(s[n // 2 - 1])) / 2.0
    return float(int(d.sum())) / float(n), float(d.max()), med


def outline_row(x, y, w, h, K):
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    K = np.asarray(K, np.int64).reshape(-1, 2)
    if len(x) == 0:
        return np.zeros(6)
    rr = roi_radius(x, y, K)
    return np.array([boxcount_fd(x, y, w, h), perimeter_fd(K), euler_number(x, y, w, h)] + (list(rr) if rr else [np.nan] * 3))


def outline_table(b, contours=None):
    """(n_roi, 6) table of a HostBatch in NAMES order (NaN: undefined in the reference)."""
    if contours is None:
        contours = contours_of(b)
    off = np.asarray(b.px_offset).astype(np.int64)
    return np.array([outline_row(b.x[off[r]:off[r + 1]], b.y[off[r]:off[r + 1]], int(b.bbox_w[r]), int(b.bbox_h[r]), contours[r])
                     for r in range(b.n_roi)]).reshape(b.n_roi, 6)


def split_columns(names):
    idx = {c: i for i, c in enumerate(names)}
    return [idx[c] for c in NAMES]
