"""The identities behind the robust statistics of roi_features.hip (16-bit-table launches), against brute force.

In offsets x = v - vmin, with C(i) = #(x <= i), F(i) = sum_{j <= i} j c_j, C(-1) = F(-1) = 0 and Xtot = sum x = F(range):

    Sx = sum of x inside [lox, hix] = F(hix) - F(lox - 1),   K = C(hix) - C(lox - 1)
    sum |x - kmed| = [kmed C(kmed) - F(kmed)] + [(Xtot - F(kmed)) - kmed (n - C(kmed))]      (both brackets >= 0)
    t = floor(Sx / K) lies in [lox, hix]                                                       (K > 0)
    sum over [lox, hix] of |K x - Sx| = 2 (Sx n1 - K S1),   n1 = C(t) - C(lox - 1),  S1 = F(t) - F(lox - 1)

and in a 16-bit-table launch (n < 65536, range < 16384): F < 2^30, K S1 and Sx n1 < 2^46, the last sum < 2^47 -- exact in 64-bit
integers and as doubles.  Checked at the points the kernel derives from the percentiles and the median (robust_prefix_cases.points)
and at random ones."""
import numpy as np
import pytest

from tests import robust_prefix_cases as rp

SIZES = (1, 2, 3, 5, 8, 40, 97, 256, 257, 600)


def check_identities(x, R, lox, hix, kmed):
    """x: offsets (int64) of a sample of range R.  Python integers throughout: no overflow can hide a mismatch."""
    n = len(x)
    C, F = rp.tables(x, R)
    xtot = int(F[R])
    assert xtot == int(x.sum()) and int(C[R]) == n
    assert xtot < 2 ** 30
    inside = x[(x >= lox) & (x <= hix)]
    K, Sx = rp.at(C, hix) - rp.at(C, lox - 1), rp.at(F, hix) - rp.at(F, lox - 1)
    assert K == len(inside) and Sx == int(inside.sum())
    below = kmed * rp.at(C, kmed) - rp.at(F, kmed)
    above = (xtot - rp.at(F, kmed)) - kmed * (n - rp.at(C, kmed))
    assert below >= 0 and above >= 0
    assert below + above == int(np.abs(x - kmed).sum())
    assert below + above < 2 ** 31
    if K:
        t = Sx // K
        assert lox <= t <= hix
        assert t == int(np.float64(Sx) / np.float64(K))            # the kernel's one fp64 division, truncated
        n1, S1 = rp.at(C, t) - rp.at(C, lox - 1), rp.at(F, t) - rp.at(F, lox - 1)
        assert Sx * n1 < 2 ** 46 and K * S1 < 2 ** 46
        adin = 2 * (Sx * n1 - K * S1)
        assert 0 <= adin < 2 ** 47
        assert adin == sum(abs(K * int(xi) - Sx) for xi in inside)
        assert float(adin) == adin                                  # exact as a double


@pytest.mark.parametrize("R", rp.RANGES)
def test_identities_match_brute_force(R):
    rng = np.random.default_rng(1000 + R)
    count = 0
    for dist, r, v in rp.samples(SIZES, seed=7):
        if r != R:
            continue
        x = np.asarray(v, np.int64) - int(np.min(v))
        Rv = int(x.max())
        assert Rv == (R if len(v) > 1 else 0)
        p = rp.points(v)
        if not p["empty"]:
            check_identities(x, Rv, p["lox"], p["hix"], p["kmed"])
        for _ in range(6):                                          # any lox <= hix and any kmed of the value domain
            lo, hi = sorted(int(q) for q in rng.integers(0, Rv + 1, 2))
            check_identities(x, Rv, lo, hi, int(rng.integers(0, Rv + 1)))
        check_identities(x, Rv, 0, Rv, p["kmed"])                   # the whole range: K = n
        count += 1
    assert count >= len(rp.DISTRIBUTIONS) * len(SIZES)


def test_bounds_at_the_limits_of_a_16_bit_table_launch():
    """65535 values over the range 16383, as many of them at the upper end as the bounds allow."""
    R, n = 16383, 65535
    for hi_share in (1.0, 0.5):
        x = np.zeros(n, np.int64)
        x[1: 1 + int((n - 1) * hi_share)] = R
        for lox, hix, kmed in ((0, R, R), (0, R, R // 2), (1, R, R - 1), (0, R - 1, 0)):
            check_identities(x, R, lox, hix, kmed)
