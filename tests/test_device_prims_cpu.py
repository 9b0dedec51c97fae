"""Keeps tests/device_prims_ref.py honest without a GPU: the restatements that tests/test_device_prims_gpu.py holds the device
primitives to are themselves checked here against something independent -- math.log2, the C oracle's exported binning, hand-computed
boundary cases, np.sum / np.cumsum / np.minimum.accumulate, Python integers, mpmath."""
import ctypes as C
import math
import struct

import numpy as np

from oracle import pyoracle as po
from tests import device_prims_ref as R

# fast_log2f against log2: the quadratic fit's own error, not a rounding matter.  Measured here over [1e-16, 1e6] (2^22 log-uniform
# points + every float within 64 ulp of the break points 0.75 * 2^k, 1.0 * 2^k, 1.5 * 2^k): worst |fast_log2f(x) - log2(x)| =
# 8.9444e-3, at x = 0.75 * 2^-52 -- the fit's own error at the break point 0.75 (log2(0.75) against 1 + a / 16 - b / 4 - 1: 8.941e-3)
# plus the float32 rounding of the sum at |lg2| = 52 (half an ulp: 1.9e-6 per operation).  The bound asserted is 9.2e-3: the measured
# worst plus a margin of 2.6e-4 (about 3 %), some sixty times the rounding and far below any other plausible fit.
LOG2_FIT_BOUND = 9.2e-3


def _log2_points():
    rng = np.random.default_rng(11)
    x = np.exp(rng.uniform(math.log(1e-16), math.log(1e6), 1 << 22))
    ks = np.arange(-54, 21)
    near = []
    for m in (0.75, 1.0, 1.5):
        c = (m * 2.0 ** ks).astype(np.float32)
        for d in range(-64, 65):
            near.append((c.view(np.uint32).astype(np.int64) + d).astype(np.uint32).view(np.float32).astype(np.float64))
    x = np.concatenate([x] + near)
    return x[(x >= 1e-16) & (x <= 1e6)]


def test_fast_log2f_is_the_quadratic_fit_of_log2():
    """oracle/nyx_oracle.c keeps its fast_log10 static, so the restatement is held to math.log2: within LOG2_FIT_BOUND (see above
    for the measured 8.9444e-3), exact at powers of two (signif - 1 = 0), and the float32 steps by hand at 1.5 (the `greater` branch:
    0.75 * 2)."""
    x = _log2_points()
    got = R.fast_log2f(x).astype(np.float64)
    err = np.abs(got - np.log2(x.astype(np.float32).astype(np.float64)))
    worst = int(err.argmax())
    print(f"fast_log2f vs log2: {len(x)} points, worst |error| {err.max():.4e} at x = {x[worst]!r}")
    assert err.max() <= LOG2_FIT_BOUND
    assert err.max() >= 8.9e-3                                         # (the measurement sees the fit's extremum at all)
    k = np.arange(-126, 128)
    assert (R.fast_log2f(2.0 ** k) == k.astype(np.float32)).all()
    f = np.float32
    s = f(0.75) - f(1.0)
    by_hand = (f(1.0) + (f(-.6296735) * s) * s) + f(1.466967) * s
    assert R.fast_log2f(np.array([1.5]))[0] == by_hand and R.fast_log2f(np.array([1.5])).dtype == np.float32
    # the double is rounded to float first: a double just below 2 that rounds up to 2.0f gives exactly 1
    assert R.fast_log2f(np.array([np.nextafter(2.0, 0.0)]))[0] == f(1.0)
    p, arg = np.array([0.25, 0.5]), np.array([0.25, 1.0])
    assert (R.plogp(p, arg) == p * R.fast_log2f(arg + 1e-9).astype(np.float64)).all()


def test_fast_log2f_scalar_bit_steps():
    """An independent scalar walk through the bit manipulation (struct, Python ints) on random floats."""
    rng = np.random.default_rng(12)
    xs = np.exp(rng.uniform(math.log(1e-16), math.log(1e6), 2000))
    got = R.fast_log2f(xs)
    f = np.float32
    for x, g in zip(xs, got):
        ui = struct.unpack("<I", struct.pack("<f", float(f(x))))[0]
        e = (ui & 0x7F800000) >> 23
        if ui & 0x00400000:
            sig = struct.unpack("<f", struct.pack("<I", (ui & 0x007FFFFF) | 0x3F000000))[0]
            fexp = f(e) - f(126.0)
        else:
            sig = struct.unpack("<f", struct.pack("<I", (ui & 0x007FFFFF) | 0x3F800000))[0]
            fexp = f(e) - f(127.0)
        s = f(sig) - f(1.0)
        want = f(f(fexp + f(f(f(-.6296735) * s) * s)) + f(f(1.466967) * s))
        assert g == want, (x, g, want)


def _oracle_bin_pixel():
    lib = po.oracle_lib()
    fn = lib.nyxo_bin_pixel
    fn.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    fn.restype = C.c_uint32
    return fn


def test_binning_restatements_match_the_oracle():
    """nyxo_bin_pixel is the oracle's exported binning (matlab for a positive grey depth, radiomics for a negative one, identity for
    0).  Random x in [mn, mx] plus 0, mn, mx, for the depths, bin counts, maxima and minima the GPU test walks."""
    fn = _oracle_bin_pixel()
    rng = np.random.default_rng(13)
    n = 0
    for info in (1, 2, 3, 8, 16, 17, 63, 64, 100, 255, 256, 4094, -1, -8, -16, -20, -24, 0):
        for mx in (1, 2, 255, 256, 4095, 65535, 2 ** 24 - 1, 2 ** 24, 2 ** 32 - 1):
            for mn in sorted({0, 1, mx - 1}):
                if info < 0 and mx == mn:
                    continue
                x = np.concatenate([[0, mn, mx], rng.integers(mn, mx + 1, 40)]).astype(np.uint32)
                got = R.bin_pixel(x, np.full_like(x, mn), np.full_like(x, mx), np.full(len(x), info))
                want = np.array([fn(int(v), mn, mx, info) for v in x], np.uint32)
                assert (got == want).all(), (info, mx, mn, x[got != want][:5])
                if info > 0:
                    direct = R.bin_matlab(x, np.full(len(x), R.matlab_slope(mx, info)), np.full(len(x), info))
                    assert (direct == want).all()
                if info < 0:
                    assert (R.bin_radiomix(x, np.full_like(x, mn), np.full_like(x, mx), np.full(len(x), -info)) == want).all()
                n += len(x)
    print(f"binning restatements: {n} values against nyxo_bin_pixel")


def test_binning_boundaries_by_hand():
    """Level boundaries worked out by hand.  matlab, 8 levels, max 255: slope = 8 / 255, level = floor(slope x + 1) clipped to
    [1, 8]; x = 32 is the first pixel of level 2 (32 * 8 / 255 = 1.0039), x = 31 the last of level 1, x = 255 would be level 9 and is
    clipped.  radiomics, 8 bins over [10, 90]: width 10; x = 19 -> 1, x = 20 -> 2, x = 90 -> 9 clipped to 8, x = 0 -> 0.
    to_grayscale: (i - min) / range * levels truncated; range 0 gives NaN, which is 0."""
    s = R.matlab_slope(255, 8)
    assert list(R.bin_matlab([0, 1, 31, 32, 63, 64, 254, 255], np.full(8, s), np.full(8, 8))) == [1, 1, 1, 2, 2, 3, 8, 8]
    x = np.array([0, 10, 19, 20, 89, 90], np.uint32)
    assert list(R.bin_radiomix(x, np.full_like(x, 10), np.full_like(x, 90), np.full(6, 8))) == [0, 1, 1, 2, 8, 8]
    assert list(R.bin_pixel(x, np.full_like(x, 10), np.full_like(x, 90), np.zeros(6, np.int64))) == list(x)
    i = np.array([5, 6, 105, 55, 7], np.uint32)
    assert list(R.to_grayscale(i, [5, 5, 5, 5, 7], [100, 100, 100, 100, 0], [8, 8, 8, 8, 8])) == [0, 0, 8, 4, 0]
    # an exact boundary: 64 levels over max 4096 - slope 2^-6 is exact, x = 64 k sits on level k + 1 exactly
    s = R.matlab_slope(4096, 64)
    assert list(R.bin_matlab([63, 64, 65, 127, 128, 4096], np.full(6, s), np.full(6, 64))) == [1, 2, 2, 2, 3, 64]


def test_integer_models_against_python_integers():
    rng = np.random.default_rng(14)
    a = rng.integers(0, 2 ** 24, 500)
    b = rng.integers(0, 2 ** 24, 500)
    c = rng.integers(0, 2 ** 32, 500)
    assert [int(v) for v in R.mul24(a, b)] == [(int(p) * int(q)) & 0xFFFFFFFF for p, q in zip(a, b)]
    assert [int(v) for v in R.mad24(a, b, c)] == [(int(p) * int(q) + int(r)) & 0xFFFFFFFF for p, q, r in zip(a, b, c)]

    def sx(v):
        v &= 0xFFFFFF
        return v - (1 << 24) if v & 0x800000 else v
    assert [int(v) for v in R.mul_i24(a, b)] == [(sx(int(p)) * sx(int(q))) & 0xFFFFFFFF for p, q in zip(a, b)]
    assert int(R.mul_i24([0x800000], [0x800000])[0]) == (2 ** 46) & 0xFFFFFFFF
    assert int(R.mul_i24([0xFFFFFF], [3])[0]) == 0xFFFFFFFD            # -1 * 3
    assert list(R.med3(np.array([0, 4, 5, 7, 9, 2 ** 32 - 1]), 5, 7)) == [5, 5, 5, 7, 7, 7]
    assert list(R.cnt16_word_offset([0, 1, 2, 3, 16382, 16383])) == [0, 0, 4, 4, 32764, 32764]
    w = R.rowcol_walk([7], [5], [3], 4)[0]
    assert [tuple(v) for v in w] == [(2, 1), (4, 0), (5, 2), (7, 1), (9, 0)]


def test_wave_models_against_numpy():
    rng = np.random.default_rng(15)
    v = rng.integers(0, 2 ** 20, (50, 64)).astype(np.float64)
    u = rng.integers(0, 2 ** 32, (50, 64)).astype(np.uint32)
    for row, urow in zip(v, u):
        assert (R.wave_sum(row) == np.sum(row)).all()
        assert (R.wave_scan(urow) == np.cumsum(urow.astype(np.uint64)).astype(np.uint32)).all()
        assert (R.wave_scan_min(urow) == np.minimum.accumulate(urow)).all()
        assert (R.wave_max(row) == row.max()).all()
        for q in range(4):
            assert (R.row16_sum(row)[16 * q:16 * q + 16] == np.sum(row[16 * q:16 * q + 16])).all()
            assert (R.row16_max(row)[16 * q:16 * q + 16] == np.max(row[16 * q:16 * q + 16])).all()
        assert list(R.lane_plus1(urow, 9)) == list(urow[1:]) + [9] and list(R.lane_minus1(urow, 9)) == [9] + list(urow[:-1])
        assert list(R.wave_rol1(urow)) == list(urow[1:]) + [urow[0]] and list(R.wave_ror1(urow)) == [urow[63]] + list(urow[:-1])
        assert (R.readlane(urow, 17) == urow[17]).all()
    assert (R.wave_sum(v) == v.sum(axis=1, keepdims=True)).all()
    for k in (4, 8, 16, 64):
        t = rng.integers(0, 2 ** 20, (6, k, 64)).astype(np.float64)
        got = R.wave_transpose_sum(t)
        shift = {4: 4, 8: 3, 16: 2, 64: 0}[k]
        for c in range(6):
            for lane in range(64):
                assert got[c, lane] == np.sum(t[c, (lane >> shift) & (k - 1)])


def test_rounding_references():
    """ordinal distance counts doubles; the longdouble-plus-mpmath route equals mpmath alone on every element."""
    one = np.array([1.0])
    assert R.ordinal_distance(np.nextafter(one, 2.0), one)[0] == 1 and R.ordinal_distance(np.nextafter(one, 0.0), one)[0] == 1
    assert R.ordinal_distance(np.array([-0.0]), np.array([0.0]))[0] == 0
    assert R.ordinal_distance(np.array([-5e-324]), np.array([5e-324]))[0] == 2
    assert R.ordinal_distance(np.array([-1.0]), np.nextafter(np.array([-1.0]), -2.0))[0] == 1
    rng = np.random.default_rng(16)
    x = np.concatenate([2.0 ** rng.uniform(-500, 500, 20000), 2.0 ** np.arange(-500.0, 501.0), np.arange(1.0, 200.0)])
    fast, n_mp = R.rsqrt_exact(x)
    slow = R.rsqrt_mp(x)
    print(f"rsqrt_exact: {n_mp} of {len(x)} elements went through mpmath")
    assert (fast == slow).all()
    assert (R.rsqrt_mp(np.array([4.0, 0.25, 2.0 ** 100])) == np.array([0.5, 2.0, 2.0 ** -50])).all()
