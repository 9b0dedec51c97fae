"""CPU model of the marginals of the fixed-order form of glcm_features_wave8 (roi_features.hip: order 8, four angles).

Lane l of an 8-lane group owns column l of the 8 x 8 count matrix P.  It sums its column from eight reads at constant offsets and
its row from one 32-byte read; the two diagonal families come from wrapped reads, one element of every row each:

  |x - y|:  d[x] = P[x][(x - l) & 7].  Rows x >= l lie on the lower diagonal l (their sum is A_l), rows x < l on the upper
            diagonal 8 - l (B_l).  dc_l = A_l + (l ? B_{8 - l} : 0); the kernel fetches the partner by a half-mirror (lane 7 - l)
            followed by a shift by one lane, into which lane 0 receives B_0 = 0 or nothing at all.
  x + y:    a[x] = P[x][(l - x) & 7].  Rows x <= l belong to k = l, rows x > l to k = l + 8; k = 15 does not exist.

The model below does what the lanes do, index by index, and is held to brute force over the cells: on random matrices, on
adversarial ones (all ones, one row, one column, either diagonal, the corners, counts near 2^32 / 64) and on the 64 matrices with
one occupied cell."""
import numpy as np
import pytest

N = 8


def lane_sums(P):
    """What the eight lanes of a group hold after the marginal step: (cc, rc, dc, ac0, ac1) as uint32 arrays indexed by lane."""
    P = np.asarray(P, np.uint32)
    w = P.reshape(-1)                                        # the count block as the kernel sees it: row-major words
    cc = np.zeros(N, np.uint32); rc = np.zeros(N, np.uint32)
    A = np.zeros(N, np.uint32); B = np.zeros(N, np.uint32)
    ac = np.zeros((2, N), np.uint32)
    with np.errstate(over="ignore"):
        for l in range(N):
            for u in range(N):
                cc[l] += w[8 * u + l]
            for j in range(N):
                rc[l] += w[8 * l + j]
            # row 0 apart ((8 - l) & 7), rows 1..7 at word 9 + 9 (x - 1) - l, + 8 where the row wraps (l > x)
            tot = up = np.uint32(0)
            d0 = w[(8 - l) & 7]
            tot += d0
            if l > 0:
                up += d0
            for x in range(1, N):
                wrap = l > x
                word = 9 - l + (8 if wrap else 0) + 9 * (x - 1)
                assert 0 <= word < 64 and word == 8 * x + ((x - l) & 7)
                tot += w[word]
                if wrap:
                    up += w[word]
            A[l], B[l] = tot - up, up
            # rows at word l + 7 x, + 8 where the row wraps (l < x)
            atot = ahi = np.uint32(0)
            for x in range(N):
                wrap = l < x
                word = l + (8 if wrap else 0) + 7 * x
                assert 0 <= word < 64 and word == 8 * x + ((l - x) & 7)
                atot += w[word]
                if wrap:
                    ahi += w[word]
            ac[0, l], ac[1, l] = atot - ahi, ahi
        # the partner: half-mirror inside the group, then a shift by one lane along the 16-lane row.  Two groups share a row: lane 0
        # of the row receives 0, lane 8 the lower group's mirrored lane 7 = its B_0
        row = np.concatenate([B, B])                         # (both groups of the row hold the same matrix here)
        mirrored = np.concatenate([row[:8][::-1], row[8:][::-1]])
        shifted = np.concatenate([[np.uint32(0)], mirrored[:-1]]).astype(np.uint32)
        dc_row = np.concatenate([A, A]) + shifted
    assert (dc_row[:8] == dc_row[8:]).all()                  # the upper group gets nothing from the lower one: B_0 = 0
    return cc, rc, dc_row[:8], ac[0], ac[1]


def brute(P):
    P = np.asarray(P, np.uint64)
    m = np.uint64(0xFFFFFFFF)
    cc = P.sum(0) & m
    rc = P.sum(1) & m
    dc = np.zeros(N, np.uint64); k = np.zeros(2 * N, np.uint64)
    for x in range(N):
        for y in range(N):
            dc[abs(x - y)] += P[x, y]
            k[x + y] += P[x, y]
    return cc, rc, dc & m, k[:8] & m, k[8:] & m


def _adversarial():
    rng = np.random.default_rng(5)
    out = [np.ones((N, N)), np.zeros((N, N)), np.eye(N), np.eye(N)[::-1], np.triu(np.ones((N, N)), 1), np.tril(np.ones((N, N)), -1)]
    for i in range(N):
        a = np.zeros((N, N)); a[i, :] = np.arange(1, 9); out.append(a)
        b = np.zeros((N, N)); b[:, i] = np.arange(1, 9); out.append(b)
        c = np.zeros((N, N)); c[np.arange(N), (np.arange(N) + i) % N] = np.arange(1, 9); out.append(c)      # a wrapped diagonal
        d = np.zeros((N, N)); d[np.arange(N), (i - np.arange(N)) % N] = np.arange(1, 9); out.append(d)      # a wrapped anti-diagonal
    out.append(np.full((N, N), (1 << 26) - 1))                                                            # sums just below 2^32
    out.append(rng.integers(0, 1 << 32, (N, N)))                                                          # sums that wrap, as uint32 does
    out += [rng.integers(0, 70000, (N, N)) for _ in range(40)] + [rng.integers(0, 3, (N, N)) for _ in range(40)]
    return out


def _check(P):
    got, want = lane_sums(P), brute(P)
    for name, g, w in zip(("column", "row", "|x - y|", "x + y (k = l)", "x + y (k = l + 8)"), got, want):
        assert (g.astype(np.uint64) == w).all(), (name, g, w, np.asarray(P))


def test_adversarial_and_random_matrices():
    for P in _adversarial():
        _check(np.asarray(P).astype(np.uint64).astype(np.uint32))


@pytest.mark.parametrize("r", range(N))
def test_one_cell_at_every_position(r):
    for c in range(N):
        P = np.zeros((N, N), np.uint32)
        P[r, c] = 7
        _check(P)
        cc, rc, dc, a0, a1 = lane_sums(P)
        assert cc[c] == 7 and rc[r] == 7 and dc[abs(r - c)] == 7 and (a0 if r + c < 8 else a1)[(r + c) & 7] == 7
        assert cc.sum() == rc.sum() == dc.sum() == 7 and a0.sum() + a1.sum() == 7


def test_k15_never_occurs():
    rng = np.random.default_rng(9)
    for _ in range(20):
        assert lane_sums(rng.integers(0, 1000, (N, N)))[4][7] == 0
