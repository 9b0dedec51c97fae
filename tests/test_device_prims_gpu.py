"""The shared device primitives of nyxus_amd/csrc/device_math.h and sort_lds.h, one by one, on an MI355X: a stand-alone probe
(tests/cpp/device_prims_probe.hip, built once per session with the library's flags) calls each of them on inputs chosen here, and
every returned value is compared with the restatements of tests/device_prims_ref.py (kept honest by tests/test_device_prims_cpu.py).

Covered: fdiv, frcp, frsq; fast_log2f, plogp; bin_radiomix, bin_matlab, bin_pixel, to_grayscale; mul24, mad24, mul_u24_su,
mad_u24_su, mul_i24, med3_u32_ss, cnt16_word; RowCol (both constructors, advance); wave_sum_t (double, u64, u32: wave_sum,
wave_sum_u64), wave_scan_u32, wave_scan_min_u32, wave_max_nonneg, wave_max_u32, row16_sum (double, u32), row16_max, lane_plus1,
lane_minus1, lane_plus1_z, lane_minus1_z, wave_rol1, wave_ror1, readlane63 (double, u64, u32), readlane_u64, readlane_f64;
wave_transpose_sum4 / 8 / 16 / 64, wave_transpose_sum8_u32; for_each_cloud_pixel<256>; radix_sort in the six instantiations of the
library.

Left out, with the reason:
* blk_sync, wav_sync, grp_sync: ordering is not observable in a unit probe (they run inside radix_sort here).
* dpp_mov0, dpp_self, dpp_perm, permlane16_swap, permlane32_swap, transpose_sum_step: covered through every user above.
* fast_log10: fast_log2f times a constant, one IEEE multiply.

Every cross-lane helper is called by full waves outside divergent control flow, as the kernels call them.  Every input stays inside
the contract its header comment states; the one exception is the printed (never asserted) line about fdiv / frcp / frsq for |b|
outside [2^-500, 2^500], which is arithmetic only."""
import os
import subprocess

import numpy as np
import pytest

from tests import device_prims_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = os.path.join(ROOT, "tests", "cpp", "device_prims_probe.hip")
PROBE_BIN = os.path.join(ROOT, "tests", "cpp", "device_prims_probe.bin")
HEADERS = [os.path.join(ROOT, "nyxus_amd", "csrc", h) for h in ("device_math.h", "sort_lds.h")]
# the library's flags (nyxus_amd/csrc/Makefile): contraction changes the binning results
HIPCC_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off"]
U32, F64 = np.uint32, np.float64


def build_probe():
    newest = max(os.path.getmtime(p) for p in [PROBE_SRC] + HEADERS)
    if not os.path.exists(PROBE_BIN) or os.path.getmtime(PROBE_BIN) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc"] + HIPCC_FLAGS + ["-o", PROBE_BIN, PROBE_SRC], check=True, capture_output=True, text=True)
    return PROBE_BIN


@pytest.fixture(scope="module")
def probe():
    return build_probe()


def _write(path, arrays):
    with open(path, "wb") as fh:
        fh.write(np.uint64(len(arrays)).tobytes())
        for a in arrays:
            raw = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
            fh.write(np.uint64(len(raw)).tobytes())
            fh.write(raw + b"\0" * (-len(raw) % 8))


def _read(path):
    raw = open(path, "rb").read()
    n, pos, out = int(np.frombuffer(raw, np.uint64, 1, 0)[0]), 8, []
    for _ in range(n):
        nb = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
        out.append(raw[pos + 8:pos + 8 + nb])
        pos += 8 + nb + (-nb % 8)
    return out


def run(probe, tmp_path, op, arrays, dtypes, timeout=60):
    """One subprocess: `probe op request result`; the result arrays as numpy arrays of `dtypes`."""
    fin, fout = str(tmp_path / "request.bin"), str(tmp_path / "result.bin")
    _write(fin, arrays)
    try:
        r = subprocess.run([probe, op, fin, fout], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        pytest.exit(f"device_prims_probe {op} did not finish in {timeout} s: nothing more is started on the GPU", returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139):
        # the probe died (abort, segmentation fault, GPU memory fault): the session ends here
        pytest.exit(f"device_prims_probe {op} died with status {r.returncode}: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0, (op, r.returncode, r.stderr[-2000:])
    got = _read(fout)
    assert len(got) == len(dtypes), (op, len(got))
    return [np.frombuffer(g, d) for g, d in zip(got, dtypes)]


# ---- fdiv, frcp, frsq ---------------------------------------------------------------------------------------------------------------
def _signs(rng, n):
    return np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)


def _around_powers(exps):
    p = 2.0 ** np.asarray(exps, F64)
    return np.concatenate([p, np.nextafter(p, 0.0), np.nextafter(p, np.inf)])


def _denominators(rng):
    """positive denominators inside the contract: log-uniform over [2^-500, 2^500], the integers the kernels divide by (1..4096,
    pixel counts up to 2^20, 1 + k), powers of two and their neighbours"""
    rand = 2.0 ** rng.uniform(-500.0, 500.0, 1_000_000)
    counts = np.arange(1, 2 ** 20 + 1, dtype=F64)
    one_plus_k = 1.0 + np.concatenate([np.arange(0, 4096, dtype=F64), rng.uniform(0.0, 255.0, 4096), rng.uniform(0.0, 1.0, 4096) ** 4])
    pw = _around_powers(np.arange(-500, 501))
    pw = pw[(pw >= 2.0 ** -500) & (pw <= 2.0 ** 500)]
    return rand, counts, one_plus_k, pw


def _report(name, got, want, label):
    d = R.ordinal_distance(got, want)
    share, worst = float((d == 0).mean()), int(d.max())
    print(f"{name} [{label}]: {d.size} results, {100 * share:.4f} % correctly rounded, worst ordinal distance {worst}")
    return d, share, worst


def _outside(rng):
    e = np.concatenate([rng.uniform(-1020.0, -500.5, 2000), rng.uniform(500.5, 1020.0, 2000)])
    return 2.0 ** e


def test_fdiv_is_within_one_ulp(probe, tmp_path):
    """fdiv(a, b) against IEEE a / b (numpy float64: correctly rounded), as ordinal distance; the header states "within 1 ulp".
    b: finite, normal, non-zero, 2^-500 <= |b| <= 2^500, both signs; a: both signs and zero, such that the quotient is normal.
    One launch over the grid a in 0..4096 x b in 1..4096 (16.8 M quotients), one over 1.6 M pairs: 1 M log-uniform random pairs,
    sums over pixel counts up to 2^20, 1 + k, powers of two, operands one ulp either side of powers of two, a = 0.
    Measured on an MI355X: grid 16 781 312 quotients, 100 % correctly rounded, worst ordinal distance 0; pairs 1 588 174 quotients,
    100 % correctly rounded, worst ordinal distance 0.  With the function's last line (the residual correction) taken out in a
    scratch copy, the same inputs give 74.7 % (grid) and 76.4 % (pairs) correctly rounded and a worst distance of 1: the two Newton
    steps alone already meet the stated bound, the last step is what makes every measured quotient correctly rounded.
    Outside the interval (printed, not asserted; 4000 pairs with |b| down to 2^-1020 and up to 2^1020, where the reciprocal nears the
    subnormals or the overflow threshold): all 4000 within 1 as well."""
    rng = np.random.default_rng(101)
    rand, _, one_plus_k, pw = _denominators(rng)          # (the bare pixel counts serve frcp / frsq; here counts divide sums)
    n = len(rand)
    a_parts = [2.0 ** rng.uniform(-500.0, 500.0, n) * _signs(rng, n)]
    b_parts = [rand * _signs(rng, n)]
    # sums of up to 2^20 pixels of up to 32 bits (integers below 2^52) and fractional sums over a pixel count
    cnt = rng.integers(1, 2 ** 20 + 1, 400_000).astype(F64)
    a_parts += [np.floor(rng.uniform(0.0, 2.0 ** 32, 200_000) * cnt[:200_000]), rng.uniform(-1e9, 1e9, 200_000)]
    b_parts += [cnt]
    k = len(one_plus_k)
    a_parts += [rng.uniform(-4096.0, 4096.0, k)]
    b_parts += [one_plus_k]
    # powers of two and their neighbours, crossed
    sub = _around_powers(np.arange(-500, 501, 25))
    sub = sub[(sub >= 2.0 ** -500) & (sub <= 2.0 ** 500)]
    A, B = np.meshgrid(np.concatenate([sub, -sub]), np.concatenate([pw[::7], -pw[::11]]), indexing="ij")
    a_parts += [A.ravel(), np.zeros(len(pw)), np.zeros(len(pw))]
    b_parts += [B.ravel(), pw, -pw]
    a, b = np.concatenate(a_parts), np.concatenate(b_parts)
    q = R.div_exact(a, b)
    assert (np.abs(b) >= 2.0 ** -500).all() and (np.abs(b) <= 2.0 ** 500).all()
    assert ((q == 0) | ((np.abs(q) >= 2.0 ** -1022) & np.isfinite(q))).all()
    ga = np.arange(0, 4097, dtype=F64)
    gb = np.arange(1, 4097, dtype=F64)
    # the out-of-contract tail rides along in the pair launch; it is cut off before anything is asserted
    ob = _outside(rng)
    oa = rng.uniform(1.0, 2.0, len(ob)) * ob
    got, = run(probe, tmp_path, "fdiv", [np.concatenate([a, oa]), np.concatenate([b, ob])], [F64])
    grid, = run(probe, tmp_path, "fdiv_grid", [ga, gb], [F64])
    d_grid, _, worst_grid = _report("fdiv", grid.reshape(len(ga), len(gb)), ga[:, None] / gb[None, :], "grid 0..4096 / 1..4096")
    d, _, worst = _report("fdiv", got[:len(a)], q, "pairs")
    i = int(d.argmax())
    print(f"fdiv worst pair: a = {a[i]!r}, b = {b[i]!r}, got {got[i]!r}, a / b = {q[i]!r}")
    do = R.ordinal_distance(got[len(a):], oa / ob)
    print(f"fdiv outside the contract (2^-1020 <= |b| < 2^-500 or 2^500 < |b| <= 2^1020, not asserted): {int((do <= 1).sum())} of {len(do)} "
          f"within 1, {int(np.isnan(got[len(a):]).sum())} NaN")
    assert worst_grid <= 1, np.argwhere(d_grid > 1)[:5]
    assert worst <= 1, (a[d > 1][:5], b[d > 1][:5])


def test_frcp_is_within_two_ulp(probe, tmp_path):
    """frcp(b) against IEEE 1 / b for positive normal b in [2^-500, 2^500]: the header states "within 1-2 ulp", the bound asserted
    is ordinal distance <= 2.  b: 1 M log-uniform, every integer 1..2^20 (pixel counts; 1..4096 among them), 1 + k, powers of two and
    the doubles one ulp either side of them.
    Measured on an MI355X: 2 063 865 reciprocals, 100 % correctly rounded, worst ordinal distance 0 (outside the interval, printed
    only: 4000 of 4000 within 2)."""
    rng = np.random.default_rng(102)
    b = np.concatenate(_denominators(rng))
    ob = _outside(rng)
    got, = run(probe, tmp_path, "frcp", [np.concatenate([b, ob])], [F64])
    d, _, worst = _report("frcp", got[:len(b)], R.rcp_exact(b), "contract")
    i = int(d.argmax())
    print(f"frcp worst: b = {b[i]!r}, got {got[i]!r}, 1 / b = {1.0 / b[i]!r}")
    do = R.ordinal_distance(got[len(b):], 1.0 / ob)
    print(f"frcp outside the contract (not asserted): {int((do <= 2).sum())} of {len(do)} within 2, {int(np.isnan(got[len(b):]).sum())} NaN")
    assert worst <= 2, b[d > 2][:5]


def test_frsq_is_within_two_ulp(probe, tmp_path):
    """frsq(x) against the correctly rounded 1 / sqrt(x) for positive normal x in [2^-500, 2^500]; bound: ordinal distance <= 2
    (the header's "within 1-2 ulp").  The reference is device_prims_ref.rsqrt_exact: np.longdouble for the bulk, and mpmath at 200
    bits, rounded once, for every element whose extended value lies within its own error of a rounding tie of the doubles -- so the
    double rounding of the longdouble route, which would otherwise shift the count of correctly rounded results by a few cases in a
    thousand, does not enter (test_device_prims_cpu.py::test_rounding_references pins the route to mpmath alone).
    Measured on an MI355X: 2 063 865 values (11 813 references through mpmath), 87.5129 % correctly rounded, worst ordinal
    distance 1 (outside the interval, printed only: 4000 of 4000 within 2)."""
    rng = np.random.default_rng(103)
    x = np.concatenate(_denominators(rng))
    ox = _outside(rng)
    got, = run(probe, tmp_path, "frsq", [np.concatenate([x, ox])], [F64])
    want, n_mp = R.rsqrt_exact(x)
    d, _, worst = _report("frsq", got[:len(x)], want, f"contract, {n_mp} references through mpmath")
    i = int(d.argmax())
    print(f"frsq worst: x = {x[i]!r}, got {got[i]!r}, 1 / sqrt(x) = {want[i]!r}")
    do = R.ordinal_distance(got[len(x):], R.rsqrt_exact(ox)[0])
    print(f"frsq outside the contract (not asserted): {int((do <= 2).sum())} of {len(do)} within 2, {int(np.isnan(got[len(x):]).sum())} NaN")
    assert worst <= 2, x[d > 2][:5]


# ---- fast_log2f, plogp ------------------------------------------------------------------------------------------------------------------
def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _log_groups():
    rng = np.random.default_rng(104)
    g = {}
    e = np.arange(1, 255, dtype=np.uint32)[:, None] << U32(23)
    pat = np.array([0, 1, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFF], np.uint32)[None, :]
    g["exponents x significands"] = _f32((e | pat).ravel()).astype(F64)
    g["random"] = np.exp(rng.uniform(np.log(1e-16), np.log(1e6), 1 << 20))
    # doubles exactly half way between two adjacent floats, and one double-ulp either side
    f = np.concatenate([np.exp(rng.uniform(np.log(1e-16), np.log(1e6), 20000)).astype(np.float32), _f32((e | pat).ravel())[:-1]])
    tie = (f.astype(F64) + np.nextafter(f, np.float32(np.inf)).astype(F64)) / 2
    g["rounding ties"] = np.concatenate([tie, np.nextafter(tie, 0.0), np.nextafter(tie, np.inf)])
    ps = [np.array([0.0])]
    for n in range(1, 4097):
        k = np.arange(0, n + 1) if n <= 256 else np.unique(np.concatenate([[0, 1, n - 1, n], rng.integers(0, n + 1, 64)]))
        ps.append(k.astype(F64) / float(n))
    p = np.concatenate(ps)
    g["glcm p + 1e-9"] = p + 0.000000001
    g["glcm p + 2.2e-16"] = p + 2.2e-16
    sub = np.concatenate([[0], 1 << np.arange(0, 23), (1 << np.arange(1, 24)) - 1, [0x400000, 0x400001, 0x3FFFFF], rng.integers(1, 1 << 23, 1000)])
    subf = _f32(sub.astype(np.uint32)).astype(F64)
    g["zero and subnormals"] = np.concatenate([subf, 2.0 ** rng.uniform(-149.0, -126.0, 1000), 2.0 ** rng.uniform(-200.0, -150.0, 50)])
    return g, p


def test_fast_log2f_and_plogp_bits(probe, tmp_path):
    """fast_log2f(x) and plogp(p, arg) return the bits of the restatement (device_prims_ref.fast_log2f: the float32 steps of the
    reference's fast_log10 up to its lg2) on: every normal float32 exponent (1..254; 255 is inf / NaN, outside the callers' range)
    with the significands 0, 1, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFF (the code branches on bit 0x400000); 2^20 random values in
    [1e-16, 1e6]; doubles exactly on a float rounding tie and one double-ulp either side; the GLCM arguments p + 1e-9 and
    p + 2.2e-16 for p = k / N (N in 1..4096: every k for N <= 256, k in {0, 1, N - 1, N} and 64 random k above); zero and float
    subnormals (float bit patterns and doubles that round into them).  plogp(p, p) on the GLCM fractions is p times the float.
    Measured on an MI355X: no group differs, the subnormal one included (the build keeps float32 denormals: nothing is flushed)."""
    groups, p = _log_groups()
    names = list(groups)
    x = np.concatenate([groups[k] for k in names])
    got, = run(probe, tmp_path, "fast_log2f", [x], [np.float32])
    want = R.fast_log2f(x)
    pos = 0
    bad = {}
    for k in names:
        n = len(groups[k])
        ne = got[pos:pos + n].view(np.uint32) != want[pos:pos + n].view(np.uint32)
        print(f"fast_log2f [{k}]: {n} values, {int(ne.sum())} differ")
        if ne.any():
            j = pos + int(np.flatnonzero(ne)[0])
            bad[k] = (int(ne.sum()), float(x[j]), float(got[j]), float(want[j]))
        pos += n
    assert not bad, bad
    gp, = run(probe, tmp_path, "plogp", [p, p], [F64])
    wp = R.plogp(p, p)
    assert (gp.view(np.uint64) == wp.view(np.uint64)).all(), p[gp.view(np.uint64) != wp.view(np.uint64)][:5]


# ---- binning --------------------------------------------------------------------------------------------------------------------------
DEPTHS = (1, 2, 3, 8, 16, 17, 63, 64, 100, 255, 256, 4094)
BIN_COUNTS = (1, 8, 16, 20, 24)
MAXIMA = (1, 2, 255, 256, 4095, 65535, 2 ** 24 - 1, 2 ** 24, 2 ** 32 - 1)


def _xs(rng, mn, mx, lo, span, n):
    """0, mn, mx, every integer within +-1 of the real-valued boundaries lo + j * span / n (j = 1..n), 1000 random values; all but the
    0 inside [mn, mx]"""
    j = np.arange(1, n + 1, dtype=F64)
    xb = np.floor(lo + j * (span / n)).astype(np.int64)
    cand = np.concatenate([xb - 1, xb, xb + 1, xb + 2, [mn, mx], rng.integers(mn, mx + 1, 1000)])
    cand = np.unique(cand[(cand >= mn) & (cand <= mx)])
    return np.concatenate([[0], cand]).astype(np.uint32)


def _bin_cases(kind):
    """(x, p1 = mn, p2 = mx, p3 = parameter) over every combination of the module's depth / count / maximum / minimum sets"""
    rng = np.random.default_rng(105)
    X, P1, P2, P3 = [], [], [], []
    params = DEPTHS if kind in ("matlab", "gray") else BIN_COUNTS
    for prm in params:
        for mx in MAXIMA:
            for mn in sorted({0, 1, mx - 1}):
                if kind == "radiomix" and mx == mn:
                    continue                                # binW = 0: left out (see the test's docstring)
                if kind == "matlab":
                    x = _xs(rng, mn, mx, 0.0, float(mx), prm)            # slope x + 1 integer: x = j mx / n
                else:
                    x = _xs(rng, mn, mx, float(mn), float(mx - mn), prm)
                if kind == "gray":
                    x = x[x >= mn]                          # i - min_i does not wrap in the callers
                    if mx == mn:
                        x = np.array([mn], np.uint32)       # range 0: only i = min exists
                X.append(x); P1.append(np.full(len(x), mn, np.uint32)); P2.append(np.full(len(x), mx, np.uint32)); P3.append(np.full(len(x), prm, np.int32))
    return np.concatenate(X), np.concatenate(P1), np.concatenate(P2), np.concatenate(P3)


def _same(got, want, *cols):
    ne = got != want
    assert not ne.any(), (int(ne.sum()), [c[ne][:5] for c in cols], got[ne][:5], want[ne][:5])


def test_binning_bits(probe, tmp_path):
    """bin_matlab, bin_radiomix, bin_pixel and to_grayscale return exactly what the float64 restatements return, for grey depths
    {1, 2, 3, 8, 16, 17, 63, 64, 100, 255, 256, 4094}, radiomics bin counts {1, 8, 16, 20, 24}, maxima {1, 2, 255, 256, 4095, 65535,
    2^24 - 1, 2^24, 2^32 - 1}, minima {0, 1, max - 1}; per combination x = 0, mn, mx, every x within +-1 of a real-valued level
    boundary (where slope * x + 1.0, or (x - mn) / binW + 1, is an integer: there contraction or another rounding would move the
    pixel to another level), and 1000 random values.  to_grayscale with range 0 returns 0 (the NaN rule).  bin_radiomix with
    mx == mn is left out: its bin width is 0 and the quotient inf or NaN; the kernels never reach it (the degenerate-ROI guards
    answer a constant ROI, and the soft-NaN tests cover that case)."""
    # matlab: through bin_pixel (positive depth) and directly with the slope the callers pass
    x, mn, mx, d = _bin_cases("matlab")
    z = np.zeros(len(x), F64)
    got, = run(probe, tmp_path, "bin_pixel", [x, mn, mx, d, z], [U32])
    _same(got, R.bin_pixel(x, mn, mx, d), x, mx, d)
    slope = R.matlab_slope(mx, d)
    got, = run(probe, tmp_path, "bin_matlab", [x, mn, mx, d, slope], [U32])
    _same(got, R.bin_matlab(x, slope, d), x, mx, d)
    n_m = len(x)
    # identity
    got, = run(probe, tmp_path, "bin_pixel", [x[:4096], mn[:4096], mx[:4096], np.zeros(4096, np.int32), z[:4096]], [U32])
    _same(got, x[:4096], x[:4096])
    # radiomics: through bin_pixel (negative count) and directly
    x, mn, mx, c = _bin_cases("radiomix")
    z = np.zeros(len(x), F64)
    got, = run(probe, tmp_path, "bin_pixel", [x, mn, mx, -c, z], [U32])
    _same(got, R.bin_pixel(x, mn, mx, -c.astype(np.int64)), x, mn, mx, c)
    got, = run(probe, tmp_path, "bin_radiomix", [x, mn, mx, c, z], [U32])
    _same(got, R.bin_radiomix(x, mn, mx, c), x, mn, mx, c)
    n_r = len(x)
    # to_grayscale(i, min, range, levels)
    x, mn, mx, d = _bin_cases("gray")
    z = np.zeros(len(x), F64)
    rg = mx - mn
    got, = run(probe, tmp_path, "to_grayscale", [x, mn, rg, d, z], [U32])
    _same(got, R.to_grayscale(x, mn, rg, d), x, mn, rg, d)
    assert (rg == 0).any() and (got[rg == 0] == 0).all()
    print(f"binning: {n_m} matlab, {n_r} radiomics, {len(x)} to_grayscale values")


# ---- 24-bit arithmetic -------------------------------------------------------------------------------------------------------------------
EDGE24 = np.array([0, 1, 2, 2 ** 12, 2 ** 16 - 1, 2 ** 16, 2 ** 23, 2 ** 24 - 1], np.uint32)
ADDENDS = np.array([0, 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32 - 2 ** 24, 0x80000001, 12345], np.uint32)


def test_24_bit_multiplies(probe, tmp_path):
    """mul24, mad24, mul_i24 (per-lane operands) and mul_u24_su, mad_u24_su (the uniform operand is a kernel argument) return the
    low 32 bits of the exact product (plus addend): operands {0, 1, 2, 2^12, 2^16 - 1, 2^16, 2^23, 2^24 - 1} crossed with each other
    and with addends that carry past 32 bits, plus 2^16 random pairs.  mul_i24 sign-extends both factors from bit 23: the same set
    (2^23 is -2^23 there, 2^24 - 1 is -1) plus +-(2^23 - 1) and -2^23 as 32-bit two's complement."""
    rng = np.random.default_rng(106)
    A, B, Cc = (v.ravel() for v in np.meshgrid(EDGE24, EDGE24, ADDENDS, indexing="ij"))
    a = np.concatenate([A, rng.integers(0, 2 ** 24, 2 ** 16)]).astype(np.uint32)
    b = np.concatenate([B, rng.integers(0, 2 ** 24, 2 ** 16)]).astype(np.uint32)
    c = np.concatenate([Cc, rng.integers(0, 2 ** 32, 2 ** 16)]).astype(np.uint32)
    signed = np.array([2 ** 23 - 1, -(2 ** 23 - 1), -2 ** 23, -1, -2], np.int64).astype(np.int32).view(np.uint32)
    sa, sb = (v.ravel() for v in np.meshgrid(np.concatenate([EDGE24, signed]), np.concatenate([EDGE24, signed]), indexing="ij"))
    a2, b2 = np.concatenate([a, sa]), np.concatenate([b, sb])
    c2 = np.concatenate([c, np.zeros(len(sa), np.uint32)])
    # (the unsigned forms see only the operands below 2^24: the signed extras are compared for mul_i24 alone)
    mul, mad, imul = run(probe, tmp_path, "i24", [a2, b2, c2], [U32, U32, U32])
    n = len(a)
    _same(mul[:n], R.mul24(a, b), a, b)
    _same(mad[:n], R.mad24(a, b, c), a, b, c)
    _same(imul, R.mul_i24(a2, b2), a2, b2)
    # wave-uniform forms: 8 edge values + 56 random as the uniform operand, each against the edge set + 1016 random lanes
    bu = np.concatenate([EDGE24, rng.integers(0, 2 ** 24, 56)]).astype(np.uint32)
    la = np.concatenate([EDGE24, rng.integers(0, 2 ** 24, 1016)]).astype(np.uint32)
    lc = np.concatenate([np.resize(ADDENDS, 8), rng.integers(0, 2 ** 32, 1016)]).astype(np.uint32)
    smul, smad = run(probe, tmp_path, "u24_su", [la, lc, bu], [U32, U32])
    _same(smul.reshape(len(bu), len(la)), R.mul24(la[None, :], bu[:, None]))
    _same(smad.reshape(len(bu), len(la)), R.mad24(la[None, :], bu[:, None], lc[None, :]))
    # every addend against every edge pair for the uniform form as well
    la2, lc2 = (v.ravel() for v in np.meshgrid(EDGE24, ADDENDS, indexing="ij"))
    smul, smad = run(probe, tmp_path, "u24_su", [la2, lc2, EDGE24], [U32, U32])
    _same(smul.reshape(len(EDGE24), len(la2)), R.mul24(la2[None, :], EDGE24[:, None]))
    _same(smad.reshape(len(EDGE24), len(la2)), R.mad24(la2[None, :], EDGE24[:, None], lc2[None, :]))


def test_med3_and_cnt16_word(probe, tmp_path):
    """med3_u32_ss(x, lo, hi) is the clamp of x to [lo, hi] for lo <= hi: x below, inside, on and above the bounds, lo == hi, and
    the extreme values 0 and 2^32 - 1 as x and as bounds.  cnt16_word(tab, ci) is tab + ((ci & ~1) << 1) bytes for every ci in
    0..16383."""
    rng = np.random.default_rng(107)
    bounds = [(0, 0), (0, 2 ** 32 - 1), (2 ** 32 - 1, 2 ** 32 - 1), (5, 5), (5, 9), (0, 7), (100, 2 ** 31), (2 ** 31, 2 ** 31 + 1), (2 ** 31 - 1, 2 ** 32 - 2), (1, 2 ** 16)]
    xs = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
    for lo, hi in bounds:
        xs += [lo - 1, lo, lo + 1, (lo + hi) // 2, hi - 1, hi, hi + 1]
    x = np.unique(np.concatenate([np.array([v for v in xs if 0 <= v < 2 ** 32], np.int64), rng.integers(0, 2 ** 32, 1000)])).astype(np.uint32)
    lo = np.array([p[0] for p in bounds], np.uint32)
    hi = np.array([p[1] for p in bounds], np.uint32)
    got, = run(probe, tmp_path, "med3", [x, lo, hi], [U32])
    got = got.reshape(len(bounds), len(x))
    for j, (l, h) in enumerate(bounds):
        _same(got[j], R.med3(x, l, h), x)
        _same(got[j], np.clip(x.astype(np.int64), l, h).astype(np.uint32), x)
    off, = run(probe, tmp_path, "cnt16", [np.array([16384], np.uint32)], [U32])
    _same(off, R.cnt16_word_offset(np.arange(16384)), np.arange(16384))


# ---- RowCol ----------------------------------------------------------------------------------------------------------------------------
def test_rowcol_small_constructor_exhaustive(probe, tmp_path):
    """RowCol(first, stride, width, small_t) takes its quotients from v_rcp_f32.  Every width 1..64 against every first 0..65535
    (the stride quotient is the same formula, and the probe passes stride = first): row and column of all 4 194 304 cases equal
    divmod, and the device's own count of cases that differ from its integer division is 0."""
    rows, cols, n_bad, bad = run(probe, tmp_path, "rowcol_small", [np.array([64], np.uint32)], [np.uint16, np.uint8, U32, U32])
    first = np.arange(65536, dtype=np.int64)[None, :]
    width = np.arange(1, 65, dtype=np.int64)[:, None]
    q, r = R.rowcol(first, width)
    ne = (rows.reshape(64, 65536) != q) | (cols.reshape(64, 65536) != r)
    print(f"RowCol small_t: {ne.size} cases, {int(ne.sum())} differ from divmod; device count {int(n_bad[0])}")
    assert int(n_bad[0]) == 0 and not ne.any(), (int(n_bad[0]), bad.reshape(16, 4)[:min(16, int(n_bad[0]))], np.argwhere(ne)[:5])


def test_rowcol_general_constructor_and_advance(probe, tmp_path):
    """4096 random (first, stride, width) triples, width up to 4096, first and stride up to 2^24, each walked 128 advance() steps:
    (row, col) equals divmod(first + k * stride, width) at every step; the triples inside the small constructor's domain (first,
    stride < 2^16, width <= 64: a quarter of them by construction, plus the domain's corners) go through it as well."""
    rng = np.random.default_rng(108)
    n = 4096
    first = rng.integers(0, 2 ** 24 + 1, n)
    stride = rng.integers(0, 2 ** 24 + 1, n)
    width = rng.integers(1, 4097, n)
    q = n // 4
    first[:q], stride[:q], width[:q] = rng.integers(0, 2 ** 16, q), rng.integers(0, 2 ** 16, q), rng.integers(1, 65, q)
    corners = [(0, 0, 1), (65535, 65535, 1), (65535, 65535, 64), (65535, 0, 63), (0, 65535, 64), (2 ** 24, 2 ** 24, 4096), (2 ** 24, 2 ** 24, 1), (4095, 4096, 4096)]
    first[q:q + 8], stride[q:q + 8], width[q:q + 8] = zip(*corners)
    f, s, w = first.astype(np.uint32), stride.astype(np.uint32), width.astype(np.uint32)
    steps = np.array([128], np.uint32)
    got, = run(probe, tmp_path, "rowcol_walk", [f, s, w, steps], [U32])
    want = R.rowcol_walk(first, stride, width, 128)
    assert want.max() < 2 ** 32
    ne = got.reshape(n, 129, 2) != want
    assert not ne.any(), [(first[i], stride[i], width[i], k) for i, k, _ in np.argwhere(ne)[:5]]
    dom = (first < 2 ** 16) & (stride < 2 ** 16) & (width <= 64)
    assert dom.sum() >= q
    got, = run(probe, tmp_path, "rowcol_walk_small", [f[dom], s[dom], w[dom], steps], [U32])
    ne = got.reshape(int(dom.sum()), 129, 2) != want[dom]
    assert not ne.any(), [(first[dom][i], stride[dom][i], width[dom][i], k) for i, k, _ in np.argwhere(ne)[:5]]


# ---- reductions, scans, shifts ------------------------------------------------------------------------------------------------------------
BOUNDARY_LANES = (0, 15, 16, 31, 32, 63)     # the row boundaries of the DPP network


def _wave_inputs(kind):
    """[cases][64]: 64 one-hot cases (a single non-zero in lane s: shows which lanes receive which source), 256 random cases of
    integers below 2^20 (every sum is exact in any order), and for the integer helpers values that use all 32 bits"""
    rng = np.random.default_rng(109)
    onehot = np.zeros((64, 64), np.int64)
    onehot[np.arange(64), np.arange(64)] = 1 + np.arange(64)
    rand = rng.integers(0, 2 ** 20, (256, 64))
    if kind == "f64":
        return np.concatenate([onehot, rand]).astype(F64)
    wide = rng.integers(0, 2 ** 32, (64, 64))
    if kind == "u64":
        wide = rng.integers(0, 2 ** 58, (64, 64))
    return np.concatenate([onehot, rand, wide]).astype(np.uint64)


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint64) if v.dtype == F64 else v.astype(np.uint64)


def _wave(probe, tmp_path, name, v, aux=(0,)):
    assert v.shape[0] % 4 == 0 and v.shape[1] == 64
    got, = run(probe, tmp_path, "wave", [name.encode() + b"\0", _bits(v), np.array(aux, np.uint32)], [np.uint64])
    return got.reshape(len(aux), v.shape[0], 64)


WAVE_REDUCTIONS = {
    # name: (input kind, model over [cases][64], result is a double)
    "wave_sum": ("f64", R.wave_sum),
    "wave_sum_u64": ("u64", R.wave_sum),
    "wave_sum_u32": ("u32", lambda v: R.wave_sum(v.astype(np.uint32))),
    "wave_scan_u32": ("u32", lambda v: R.wave_scan(v.astype(np.uint32))),
    "wave_max_nonneg": ("f64", R.wave_max),
    "wave_max_u32": ("u32", R.wave_max),
    "row16_sum": ("f64", R.row16_sum),
    "row16_sum_u32": ("u32", lambda v: R.row16_sum(v.astype(np.uint32))),
    "row16_max": ("f64", R.row16_max),
    "readlane63_f64": ("f64", lambda v: R.readlane(v, 63)),
    "readlane63_u64": ("u64", lambda v: R.readlane(v, 63)),
    "readlane63_u32": ("u32", lambda v: R.readlane(v, 63)),
}


@pytest.mark.parametrize("name", list(WAVE_REDUCTIONS))
def test_wave_reductions_and_scans(probe, tmp_path, name):
    """Every lane's result is exact on 64 one-hot inputs (a single value in lane s) and 256 random inputs of integers below 2^20
    (doubles: every sum is exact in any order), plus 64 inputs that use the whole word for the integer helpers (32-bit sums wrap modulo
    2^32).  wave_max_nonneg sees non-negative inputs only: that is its contract (the lanes without a source compare
    against a 0 fill)."""
    kind, model = WAVE_REDUCTIONS[name]
    v = _wave_inputs(kind)
    got = _wave(probe, tmp_path, name, v)[0]
    want = _bits(np.ascontiguousarray(model(v)))
    ne = got != want
    assert not ne.any(), (name, [(int(c), int(l), int(got[c, l]), int(want[c, l])) for c, l in np.argwhere(ne)[:8]])


def test_wave_scan_min(probe, tmp_path):
    """wave_scan_min_u32: descending, ascending and random inputs (32-bit values, 0 and 2^32 - 1 among them), and a single minimum
    in each lane in turn."""
    rng = np.random.default_rng(110)
    single = np.full((64, 64), 1000, np.int64)
    single[np.arange(64), np.arange(64)] = 7
    desc = (2 ** 32 - 1 - np.arange(64) * 1000)[None, :]
    asc = (np.arange(64) * 67108863)[None, :]
    rand = rng.integers(0, 2 ** 32, (253, 64))
    allmax = np.full((1, 64), 2 ** 32 - 1)
    v = np.concatenate([single, desc, asc, allmax, rand]).astype(np.uint64)
    got = _wave(probe, tmp_path, "wave_scan_min_u32", v)[0]
    want = R.wave_scan_min(v)
    ne = got != want
    assert not ne.any(), [(int(c), int(l), int(got[c, l]), int(want[c, l])) for c, l in np.argwhere(ne)[:8]]


SHIFTS = {
    # name: (model(v, fill), takes the fill from the caller)
    "lane_plus1": (R.lane_plus1, True),
    "lane_minus1": (R.lane_minus1, True),
    "lane_plus1_lit0": (lambda v, f: R.lane_plus1(v, 0), False),     # lane_plus1(v, 0): the literal-zero form (bound_ctrl)
    "lane_minus1_lit0": (lambda v, f: R.lane_minus1(v, 0), False),
    "lane_plus1_z": (lambda v, f: R.lane_plus1(v, 0), False),
    "lane_minus1_z": (lambda v, f: R.lane_minus1(v, 0), False),
    "wave_rol1": (lambda v, f: R.wave_rol1(v), False),
    "wave_ror1": (lambda v, f: R.wave_ror1(v), False),
}


@pytest.mark.parametrize("name", list(SHIFTS))
def test_lane_shifts_and_rotations(probe, tmp_path, name):
    """Distinct values per lane (and the one-hot and random sets), fill values 0 and 0xDEADBEEF: every lane holds its neighbour's
    value, the lane without a source holds the fill (shifts) or the value from the other end (rotations).  Lanes 0, 15, 16, 31, 32
    and 63 -- the row boundaries of the DPP network -- are checked one by one as well."""
    model, takes_fill = SHIFTS[name]
    distinct = (0x01010000 * (1 + np.arange(64)) + np.arange(64) + 1)[None, :] ^ np.array([0, 0x5A5A5A5A, 0xFFFFFFFF, 0x80000000])[:, None]
    v = np.concatenate([distinct & 0xFFFFFFFF, _wave_inputs("u32")]).astype(np.uint64)
    assert len(np.unique(v[0])) == 64
    fills = (0, 0xDEADBEEF)
    got = _wave(probe, tmp_path, name, v, fills)
    for j, fill in enumerate(fills):
        want = model(v, fill).astype(np.uint64)
        ne = got[j] != want
        assert not ne.any(), (name, hex(fill), [(int(c), int(l), hex(int(got[j, c, l])), hex(int(want[c, l]))) for c, l in np.argwhere(ne)[:8]])
        for lane in BOUNDARY_LANES:
            src = lane + 1 if "plus1" in name or "rol" in name else lane - 1
            if 0 <= src < 64:
                exp = v[:, src]
            elif "rol" in name or "ror" in name:
                exp = v[:, src % 64]
            else:
                exp = np.full(len(v), fill if takes_fill else 0, np.uint64)
            assert (got[j][:, lane] == exp).all(), (name, lane, hex(fill))


@pytest.mark.parametrize("name", ["readlane_u64", "readlane_f64"])
def test_readlane_any_lane(probe, tmp_path, name):
    """readlane_u64 / readlane_f64 with every wave-uniform lane index 0..63 (a kernel argument) on 64-bit patterns."""
    rng = np.random.default_rng(111)
    v = rng.integers(0, 2 ** 63, (8, 64)).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    if name == "readlane_f64":
        v = rng.integers(0, 2 ** 52, (8, 64)).astype(F64) * 2.0 ** rng.integers(-300, 300, (8, 64))
    lanes = tuple(range(64))
    got = _wave(probe, tmp_path, name, v, lanes)
    b = _bits(v)
    for lane in lanes:
        assert (got[lane] == b[:, lane:lane + 1]).all(), (name, lane)


# ---- transposed sums -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,k", [("transpose4", 4), ("transpose8", 8), ("transpose8_u32", 8), ("transpose16", 16), ("transpose64", 64)])
def test_transposed_sums(probe, tmp_path, op, k):
    """wave_transpose_sum4 / 8 / 16 / 64 and wave_transpose_sum8_u32: one-hot over every (slot, lane) pair (64 k cases, one wave
    each: 4096 for the 64-slot form) and 64 random integer-valued inputs below 2^20.  Lane L returns the wave total of slot
    (L >> 4) & 3 (4 slots), (L >> 3) & 7 (8 slots, both forms), (L >> 2) & 15 (16 slots), L (64 slots): in a one-hot case exactly
    the lanes of that slot hold the value and every other lane holds 0."""
    rng = np.random.default_rng(112)
    n1 = 64 * k
    val = 1.0 + np.arange(n1, dtype=F64)
    dense = rng.integers(0, 2 ** 20, (64, k, 64)).astype(F64)
    got, = run(probe, tmp_path, op, [val, dense], [F64])
    got = got.reshape(n1 + 64, 64)
    lanes = np.arange(64)
    slot_of_lane = {4: (lanes >> 4) & 3, 8: (lanes >> 3) & 7, 16: (lanes >> 2) & 15, 64: lanes}[k]
    assert (slot_of_lane == R.transpose_slot(k)).all()
    want1 = np.where(slot_of_lane[None, :] == (np.arange(n1) >> 6)[:, None], val[:, None], 0.0)
    ne = got[:n1] != want1
    assert not ne.any(), (op, [(int(c) >> 6, int(c) & 63, int(l), float(got[c, l])) for c, l in np.argwhere(ne)[:8]])
    want = R.wave_transpose_sum(dense)
    ne = got[n1:] != want
    assert not ne.any(), (op, np.argwhere(ne)[:8])


# ---- for_each_cloud_pixel ----------------------------------------------------------------------------------------------------------------
def test_for_each_cloud_pixel_visits_every_index_once(probe, tmp_path):
    """for_each_cloud_pixel<256> over n in {0, 1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 2051}: arrays of exactly n elements
    inside a larger allocation, followed by sentinels.  Every index below n is visited exactly once with its own (v, x, y); nothing
    at or beyond n is visited (a visit there would deliver a sentinel, or the 0 of an out-of-range buffer load)."""
    rng = np.random.default_rng(113)
    ns = (0, 1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 2051)
    pad = 1032                                                  # more than one trip of the loop (4 * 256) past the end
    desc, off = [], 0
    for n in ns:
        cap = n + pad
        desc.append((off, n, cap))
        off += (cap + 7) & ~7
    tot = off
    inten = np.full(tot, 0xDEADBEEF, np.uint32)
    x = np.full(tot, 0xBEEF, np.uint16)
    y = np.full(tot, 0xDEAD, np.uint16)
    for o, n, _ in desc:
        inten[o:o + n] = rng.integers(0, 2 ** 32, n)
        x[o:o + n] = rng.integers(0, 2 ** 16, n)
        y[o:o + n] = rng.integers(0, 2 ** 16, n)
    visits, gv, gx, gy, beyond = run(probe, tmp_path, "cloud", [inten, x, y, np.array(desc, np.uint32)], [U32] * 5)
    assert (beyond == 0).all(), beyond
    for o, n, cap in desc:
        assert (visits[o:o + n] == 1).all(), (n, np.flatnonzero(visits[o:o + n] != 1)[:5])
        assert (visits[o + n:o + cap] == 0).all(), (n, np.flatnonzero(visits[o + n:o + cap])[:5])
        assert (gv[o:o + n] == inten[o:o + n]).all() and (gx[o:o + n] == x[o:o + n]).all() and (gy[o:o + n] == y[o:o + n]).all(), n
    assert int(visits.sum()) == sum(ns)


# ---- radix_sort --------------------------------------------------------------------------------------------------------------------------
# exactly the (GS, NW, KEY) combinations the library instantiates: roi_features.hip radix_sort<GS, NW, uint16_t | uint32_t> with
# GS in {false, true} at NW = 4 (256 threads) and GS = false at NW = 8 (the 512-thread launch); roi_wide.hip <false, 4, uint16_t>;
# roi_chords.hip <false, kHW = 4, uint32_t>.  GS = true: both key buffers and the digit tables are global memory.
SORT_VARIANTS = [("lds_4_u16", 4, np.uint16), ("lds_4_u32", 4, np.uint32), ("gs_4_u16", 4, np.uint16), ("gs_4_u32", 4, np.uint32),
                 ("lds_8_u16", 8, np.uint16), ("lds_8_u32", 8, np.uint32)]
SORT_RANGES = (0, 1, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 32 - 1)
SORT_KMIN = (0, 5, 3_000_000_000)
SORT_PATTERNS = ("equal", "two", "sorted", "reversed", "random")


def _sort_cases(nw, key):
    rng = np.random.default_rng(114)
    key_max = int(np.iinfo(key).max)
    ns = sorted({1, 2, 63, 64, 65, 255, 256, 257, 64 * nw - 1, 64 * nw, 64 * nw + 1, 1000, 4099})
    keys, desc, meta, off = [], [], [], 0
    for rg in SORT_RANGES:
        if rg > key_max:
            continue                                        # 16-bit keys: ranges up to 65535
        for kmin in SORT_KMIN:
            if kmin > key_max:
                continue                                    # (no 16-bit key is that large)
            hi = min(kmin + rg, key_max)                    # keys lie in [kmin, kmin + range], inside the key type
            for n in ns:
                for pat in SORT_PATTERNS:
                    if pat == "equal":
                        k = np.full(n, rng.integers(kmin, hi + 1))
                    elif pat == "two":
                        k = np.where(rng.integers(0, 2, n) == 1, hi, kmin)
                    else:
                        k = rng.integers(kmin, hi + 1, n)
                        if pat != "random":
                            k = np.sort(k)
                            if pat == "reversed":
                                k = k[::-1]
                    keys.append(k.astype(key))
                    desc.append((off, n, kmin, rg))
                    meta.append((n, kmin, rg, pat))
                    off += (n + 7) & ~7
    flat = np.zeros(off, key)
    for k, d in zip(keys, desc):
        flat[d[0]:d[0] + d[1]] = k
    return flat, np.array(desc, np.uint32), meta


@pytest.mark.parametrize("variant,nw,key", SORT_VARIANTS, ids=[v[0] for v in SORT_VARIANTS])
def test_radix_sort(probe, tmp_path, variant, nw, key):
    """One workgroup per case: n in {1, 2, 63, 64, 65, 255, 256, 257, 64 NW - 1, 64 NW, 64 NW + 1, 1000, 4099} (the probe sizes its
    key buffers to the largest, 4104 keys: 41 KB of LDS for 32-bit keys at NW = 8, so nothing is capped away), ranges {0, 1, 255, 256,
    65535, 65536, 2^24 - 1, 2^24, 2^32 - 1} (16-bit keys: up to 65535), kmin in {0, 5, 3 * 10^9} (32-bit keys; 16-bit keys cannot hold
    the last; with kmin + range past the key type the keys fill [kmin, type maximum] and `range` is passed as is), keys all equal / two
    distinct values / sorted / reversed / random.  The output equals np.sort of the input; the returned pointer is buffer a after an
    even number of passes (one per byte of the range) and b after an odd one; range 0 makes no pass: a is returned untouched."""
    flat, desc, meta = _sort_cases(nw, key)
    got, which, a_after = run(probe, tmp_path, "sort_" + variant, [flat, desc], [key, U32, key], timeout=120)
    bad = []
    for c, (n, kmin, rg, pat) in enumerate(meta):
        o = int(desc[c, 0])
        passes = (int(rg).bit_length() + 7) // 8
        if not (got[o:o + n] == np.sort(flat[o:o + n])).all():
            bad.append(("order", n, kmin, rg, pat))
        if int(which[c]) != (passes & 1):
            bad.append(("buffer", n, kmin, rg, pat, int(which[c])))
        if rg == 0 and not (a_after[o:o + n] == flat[o:o + n]).all():
            bad.append(("untouched", n, kmin, rg, pat))
    print(f"radix_sort {variant}: {len(meta)} cases, {len(flat)} keys")
    assert not bad, (len(bad), bad[:10])
