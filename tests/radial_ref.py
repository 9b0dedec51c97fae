"""NumPy restatement of the reference's RadialDistributionFeature (FRAC_AT_D, MEAN_FRAC, RADIAL_CV): own code, written
from /root/reference/src/nyx/features/radial_distribution.cpp:43-105, :212-247 and features/pixel.cpp:40-70, :116-162.

Takes a HostBatch plus the ROIs' merged contours (padded coordinates, walk order).  Without `contours` they come from the C
oracle's test hook `nyxo_contour` (oracle/nyx_oracle.c, pinned bit for bit to the reference's ContourFeature by
tests/test_oracle_golden.py).  tests/test_radial_cpu.py pins this module to tables recorded from the reference classes
(tests/golden/radial); it then serves arbitrary inputs: fuzz, mixed masks, pixel-order permutations.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

NUM_BINS = 8                 # RadialDistributionFeature::num_bins, radial_distribution.h:36
EPSILON = 0.000000001        # radial_distribution.h:71
NAMES = [f"{c}_{i}" for c in ("FRAC_AT_D", "MEAN_FRAC", "RADIAL_CV") for i in range(NUM_BINS)]
EXACT = {f"{c}_{i}" for c in ("FRAC_AT_D", "MEAN_FRAC") for i in range(NUM_BINS)} | {"FRAC_AT_D", "MEAN_FRAC"}


def contours_of(b):
    """Merged multicontour of every ROI of a HostBatch: list of (n, 2) int64 arrays, padded coordinates."""
    from oracle import pyoracle as po
    lib = po.oracle_lib()
    lib.nyxo_contour.restype = C.c_int
    lib.nyxo_contour.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]
    off = np.asarray(b.px_offset).astype(np.int64)
    out = []
    for r in range(b.n_roi):
        o, n = int(off[r]), int(off[r + 1] - off[r])
        x, y, v = (np.ascontiguousarray(a[o:o + n]) for a in (b.x, b.y, b.inten))
        buf = np.zeros((max(n, 1), 2), np.int32)
        k = lib.nyxo_contour(x.ctypes.data, y.ctypes.data, v.ctypes.data, n, int(b.bbox_w[r]), int(b.bbox_h[r]), buf.ctypes.data, len(buf))
        assert 0 <= k <= len(buf)
        out.append(buf[:k].astype(np.int64))
    return out


def _descent(px, py, K, want_max):
    """Pixel2::min_sqdist / max_sqdist v2 (pixel.cpp:40-70, :116-143): hill descent over the ordered contour.  Squared
    distances are integers here; the reference forms them in double, exactly.  A candidate replaces the incumbent only when
    strictly better, so a round's winner is the FIRST best candidate."""
    n = len(K)
    if n == 0:
        return 0

    def sqd(idx):
        dx, dy = K[idx, 0] - px, K[idx, 1] - py
        return dx * dx + dy * dy
    extrem_d, extrem_i = int(sqd(0)), 0
    if n == 1:              # (int)(1 / log(1)): the reference's first step is undefined; the point's distance comes back
        return extrem_d
    a, b = 0, n
    step = int((b - a) / math.log(b - a))
    while True:
        idx = np.arange(a + step, b, step)
        if len(idx):
            d = sqd(idx)
            j = int(np.argmax(d) if want_max else np.argmin(d))          # first occurrence of the round's best
            if (d[j] > extrem_d) if want_max else (d[j] < extrem_d):
                extrem_d, extrem_i = int(d[j]), int(idx[j])
        step_l = step if extrem_i >= step else extrem_i
        step_r = step if extrem_i + step < n else n - extrem_i
        a, b = extrem_i - step_l, extrem_i + step_r
        step = 1 if b - a <= 10 else int((b - a) / math.log(b - a))
        if not b - a > 2:
            return extrem_d


def min_sqdist(px, py, K):
    return _descent(px, py, K, False)


def max_sqdist(px, py, K):
    return _descent(px, py, K, True)


def find_center(x, y, K):
    """Pixel2::find_center (pixel.cpp:146-162): the first pixel with the smallest max_sqdist - min_sqdist."""
    best, best_i = None, 0
    for i in range(len(x)):
        dif = max_sqdist(int(x[i]), int(y[i]), K) - min_sqdist(int(x[i]), int(y[i]), K)
        if best is None or dif < best:
            best, best_i = dif, i
    return best_i


def radial_row(x, y, inten, K):
    """One ROI -> (24 values, dstOC^2).  dstOC^2 is None without a contour; 0 marks the reference's undefined case (division by
    zero, NaN converted to int) -- the row is then 24 zeros, the HIP path's stated choice."""
    n = NUM_BINS
    x, y, inten = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(inten, np.int64)
    if len(x) == 0 or len(K) == 0:                                           # :55-56
        return np.zeros(3 * n), None
    o = find_center(x, y, K)
    cx, cy = int(x[o]), int(y[o])
    d2 = max_sqdist(cx, cy, K)
    if d2 == 0:
        return np.zeros(3 * n), 0
    dst_oc = math.sqrt(float(d2))                                            # :72
    dx, dy = x - cx, y - cy
    dst_oa = np.sqrt((dx * dx + dy * dy).astype(np.float64))                 # :77
    bi = np.minimum(((dst_oa / dst_oc) * float(n - 1)).astype(np.int64), n - 1)   # :80-83
    ang = np.array([math.atan2(float(b_), float(a_)) for a_, b_ in zip(dx, dy)], np.float64)   # :92 (libm's atan2, like the reference)
    ang = np.where(ang < 0, 2.0 * math.pi + ang, ang)
    w_bin = (ang / (2.0 * math.pi / float(n))).astype(np.int64)              # :95-96
    counts = np.bincount(bi, minlength=n)[:n]
    banded = np.zeros((n, n), np.int64)                                      # size_t in the reference
    np.add.at(banded, (bi, w_bin), inten)
    inten_bins = np.zeros(n, np.float64)                                     # a vector<double> there: integer sums, exact below 2^53
    np.add.at(inten_bins, bi, inten.astype(np.float64))
    out = np.zeros(3 * n)
    out[0:n] = counts.astype(np.float64) / (float(len(x)) + EPSILON)         # :212-216
    out[n:2 * n] = inten_bins / (counts.astype(np.float64) + EPSILON)        # :218-222
    for i in range(n):                                                       # :224-247, the summation order as written
        s = 0.0
        for w in banded[i]:
            s += float(w)
        mean = s / float(n)
        s = 0.0
        for w in banded[i]:
            s += (float(w) - mean) * (float(w) - mean)
        out[2 * n + i] = math.sqrt(s / float(n)) / (mean + EPSILON)
    return out, d2


def radial_table(b, contours=None, with_dst2=False):
    """(n_roi, 24) table of a HostBatch in the column order FRAC_AT_D_0..7, MEAN_FRAC_0..7, RADIAL_CV_0..7."""
    if contours is None:
        contours = contours_of(b)
    off = np.asarray(b.px_offset).astype(np.int64)
    T = np.zeros((b.n_roi, 3 * NUM_BINS))
    D = []
    for r in range(b.n_roi):
        o, e = int(off[r]), int(off[r + 1])
        T[r], d2 = radial_row(b.x[o:e], b.y[o:e], b.inten[o:e], np.asarray(contours[r], np.int64).reshape(-1, 2))
        D.append(d2)
    return (T, D) if with_dst2 else T


def split_columns(names):
    """Indices of the 24 radial columns inside a column list of the library, in NAMES order."""
    idx = {c: i for i, c in enumerate(names)}
    return [idx[c] for c in NAMES]
