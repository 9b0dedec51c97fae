"""Samples and a numpy restatement for the robust statistics of roi_features.hip (16-bit-table launches): ROBUST_MEAN,
MEDIAN_ABSOLUTE_DEVIATION and ROBUST_MEAN_ABSOLUTE_DEVIATION are read off two prefix tables over the offsets x = v - vmin, the
counts C(i) = #(x <= i) and the first moments F(i) = sum_{j <= i} j c_j, at the points lox - 1, hix, kmed and t.

`points(v)` restates how the kernel gets there: P10 / P90 of the reference's 100-bin histogram (histogram.h:54-66, :214-243, as in
tests/test_percentile_shortcut_cpu.py) -> lox = ceil(P10) - vmin, hix = floor(P90) - vmin; the median (histogram.h:268-287) ->
kmed = floor(median) - vmin; t = floor(Sx / K).  Shared by tests/test_robust_prefix_cpu.py and tests/test_robust_prefix_gpu.py."""
import math

import numpy as np

RANGES = (0, 1, 7, 8, 9, 511, 2047, 2048, 4094, 16383)
DISTRIBUTIONS = ("uniform", "two_valued", "exponential", "constant_outliers")
BASE = 5                                  # the smallest value of every sample: offsets and values differ


def sample(dist, R, n, rng, const=None):
    """n integer values in [BASE, BASE + R]; both ends are present when n >= 2 and R > 0 (the sample's range is R), n = 1 gives BASE."""
    if n == 1 or R == 0:
        return np.full(n, BASE, np.int64)
    if dist == "uniform":
        x = rng.integers(0, R + 1, n)
    elif dist == "two_valued":            # 90 / 10 at the extremes
        x = np.where(np.arange(n) < max(1, min(n - 1, round(0.9 * n))), 0, R)
    elif dist == "exponential":
        x = np.minimum(R, rng.exponential(R / 8.0 + 0.5, n).astype(np.int64))
    elif dist == "constant_outliers":     # a constant and two outliers
        x = np.full(n, R // 2 if const is None else const)
    else:
        raise ValueError(dist)
    x = np.array(x, np.int64)
    x[0], x[-1] = 0, R
    return BASE + rng.permutation(x)


def idx100(x, R):
    """histogram.h:55-60 on offsets: the bin index in 0 .. 100 (NaN -> 0 when the range is zero)."""
    bw = np.float64(R) / np.float64(100.)
    with np.errstate(all="ignore"):
        real = np.asarray(x, np.float64) / bw
    return np.where(np.isnan(real), 0, real).astype(np.int64)


def percentile(s, frac):
    """The reference's percentile of the sorted values s: the winning bin of the 100-bin histogram (the folded last bin is 99),
    interpolated inside the bin -- in the operation order of the kernel."""
    n, vmin = len(s), int(s[0])
    R = int(s[-1]) - vmin
    bw = np.float64(R) / np.float64(100.)
    cnt = np.float64(n) * np.float64(frac)
    idx = idx100(s - vmin, R)
    win = min(99, int(idx[int(cnt)]))
    rs = int((idx < win).sum())
    bi = (n if win + 1 >= 100 else int((idx < win + 1).sum())) - rs
    return (cnt - np.float64(rs)) * bw / np.float64(bi) + np.float64(vmin) + bw * np.float64(win)


def tables(x, R):
    """(C, F) over the offsets 0 .. R."""
    c = np.bincount(x, minlength=R + 1).astype(np.int64)
    return np.cumsum(c), np.cumsum(np.arange(R + 1, dtype=np.int64) * c)


def at(T, i):
    return int(T[i]) if i >= 0 else 0


def points(v):
    """What the kernel derives for the values v: a dict with n, R, Q (table entries per wave), empty, lox, hix, kmed, half (the median
    is kmed + 1/2), K, Sx, t (None when K = 0) and `lookups`, the table indices it reads F and C at."""
    s = np.sort(np.asarray(v, np.int64))
    n, vmin, vmax = len(s), int(s[0]), int(s[-1])
    R = vmax - vmin
    x = s - vmin
    p10, p90 = percentile(s, 0.1), percentile(s, 0.9)
    empty, lox, hix = True, None, None
    if p10 <= p90 and p90 >= vmin and p10 <= vmax:
        lo_b = vmin if math.ceil(p10) <= vmin else int(math.ceil(p10))
        hi_b = vmax if math.floor(p90) >= vmax else int(math.floor(p90))
        if lo_b <= hi_b:
            empty, lox, hix = False, lo_b - vmin, hi_b - vmin
    median = float(s[n // 2]) if n & 1 else (float(s[n // 2]) + float(s[max(n // 2 - 1, 0)])) / 2.0
    m2x = int((median - vmin) * 2.0)
    kmed = m2x >> 1
    C, F = tables(x, R)
    K = Sx = 0
    t = None
    lookups = [kmed]
    if not empty:
        K = at(C, hix) - at(C, lox - 1)
        Sx = at(F, hix) - at(F, lox - 1)
        lookups.append(hix)
        if lox > 0:
            lookups.append(lox - 1)
        if K:
            t = Sx // K
            lookups.append(t)
    return dict(n=n, R=R, Q=((R + 1 + 2047) // 2048) * 512, empty=empty, lox=lox, hix=hix, kmed=kmed, half=bool(m2x & 1), K=K, Sx=Sx, t=t,
                lookups=lookups)


def samples(sizes, seed):
    """(distribution, R, values) over RANGES x DISTRIBUTIONS x sizes, and constants that put kmed on both sides of a wave-quarter
    boundary of the tables that have one (Q - 1 and Q)."""
    rng = np.random.default_rng(seed)
    for R in RANGES:
        for dist in DISTRIBUTIONS:
            for n in sizes:
                yield dist, R, sample(dist, R, n, rng)
    for R in (2047, 4094, 16383):
        Q = ((R + 1 + 2047) // 2048) * 512
        for c in (Q - 1, Q, 2 * Q - 1, 2 * Q):
            yield "constant_outliers", R, sample("constant_outliers", R, max(sizes), rng, const=c)
