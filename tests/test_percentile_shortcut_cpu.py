"""The identity behind the percentile code of roi_features.hip: the bin that wins percentile p in the reference's 100-bin histogram
(histogram.h:54-66 builds the bins, :214-243 lets the LAST bin i with runSum_i <= cnt_p <= runSum_i + bins_i win) is

    min(99, idx100(x_c)),   c = floor(n * p),   x_c the c-th smallest value (0-based),

with idx100 the reference's own bin function (NaN -> 0 when the range is zero) and 99 the last bin, into which bin 100 is folded.
The kernel takes six order statistics and twelve bin bounds instead of a hundred bounds; this file pins the identity on the CPU.

Why it holds: runSum_i is non-decreasing in i and cnt_p < n, so the winner is the largest i with runSum_i <= floor(cnt_p); runSum_i
counts the values whose bin index is below i, the bin index is monotone in the value, hence runSum_i <= c exactly when x_c has a bin
index >= i."""
import numpy as np
import pytest

FRACS = (0.01, 0.1, 0.25, 0.75, 0.9, 0.99)


def idx100(v, vmin, rng):
    """histogram.h:55-60 -- the value's bin index in 0 .. 100."""
    bw = np.float64(rng) / np.float64(100.)
    with np.errstate(all="ignore"):
        real = (np.asarray(v, np.int64) - vmin).astype(np.float64) / bw
    return np.where(np.isnan(real), 0, np.nan_to_num(real)).astype(np.int64)


def reference_winners(v):
    """The reference loop restated: bins100 with the folded last bin, then for every percentile the last matching bin (-1: none)."""
    v = np.asarray(v, np.int64)
    n, vmin = len(v), int(v.min())
    bins = np.bincount(idx100(v, vmin, int(v.max()) - vmin), minlength=101)
    bins[99] += bins[100]
    bins = bins[:100]
    run = np.concatenate(([0], np.cumsum(bins)[:-1]))           # runSum before bin i
    out = []
    for f in FRACS:
        cnt = np.float64(n) * np.float64(f)
        hit = np.nonzero((run <= cnt) & (cnt <= run + bins))[0]
        out.append(int(hit[-1]) if len(hit) else -1)
    return out


def shortcut_winners(v):
    s = np.sort(np.asarray(v, np.int64))
    n, vmin = len(s), int(s[0])
    rng = int(s[-1]) - vmin
    return [min(99, int(idx100(s[int(np.float64(n) * np.float64(f))], vmin, rng))) for f in FRACS]


def two_valued(n, R, share, rng):
    k = max(1, min(n - 1, int(round(n * share)))) if n > 1 else 0
    return rng.permutation(np.concatenate([np.full(k, 5), np.full(n - k, 5 + R)]))


def with_ends(v, lo, hi):
    v = np.array(v)
    if len(v) > 1:
        v[0], v[-1] = lo, hi
    return v


def arrays():
    """Seeded arrays over the cases of the GPU test (tests/test_percentile_order_stats_gpu.py) and random sizes between them."""
    rng = np.random.default_rng(20)
    for n in (100, 200, 400):                                   # integer cnt_p on a bin edge: 100 occupied bins of n / 100
        yield 1 + 10 * (np.arange(n) // (n // 100))
    sizes = [1, 2, 3, 4, 5, 7, 10, 50, 99, 100, 101, 200, 400, 1000, 2821]
    for n in sizes:
        for R in (1, 2, 99, 100, 101, 4094, 16383):             # empty bins around the winners
            for share in (0.5, 0.05):
                yield two_valued(n, R, share, rng)
        v = rng.integers(1, 1000, n)                            # the folded last bin: 60 % at the maximum
        v[: (6 * n + 9) // 10] = 1000
        yield v
        for R in (100, 200, 16383, 16384, 70000):               # ranges with exact real boundaries, table bounds, a wide range
            yield with_ends(rng.integers(5, 5 + R + 1, n), 5, 5 + R)
        yield np.full(n, 7)                                     # constant, all zero
        yield np.zeros(n, np.int64)
        yield rng.integers(0, 3, n)                             # ties
        yield np.concatenate([np.full(n // 2, 3), rng.integers(3, 104, n - n // 2)])   # half the pixels tied on the minimum
    for n in (2, 3, 4, 5):                                      # few pixels, distinct values
        yield 1 + 100 * rng.permutation(n)
    for t in range(3000):                                       # ordinary data at random sizes and ranges
        n = int(rng.choice(sizes))
        hi = int(rng.choice([2, 3, 10, 100, 101, 300, 4096, 16384, 65536]))
        yield rng.integers(1, hi + 1, n)


def test_winning_bin_is_the_bin_of_one_order_statistic():
    count = 0
    for v in arrays():
        want, got = reference_winners(v), shortcut_winners(v)
        assert -1 not in want, (len(v), want)                   # some bin always wins: the kernel interpolates unconditionally
        assert want == got, (len(v), int(np.min(v)), int(np.max(v)), want, got)
        count += 1
    assert count > 3000


@pytest.mark.parametrize("n", [100, 200, 400])
def test_last_matching_bin_wins_on_a_bin_edge(n):
    """cnt_p25 = n / 4 = runSum_25: bins 24 and 25 both match, and the reference keeps the last."""
    v = 1 + 10 * (np.arange(n) // (n // 100))
    assert reference_winners(v)[2] == 25
    assert shortcut_winners(v)[2] == 25
