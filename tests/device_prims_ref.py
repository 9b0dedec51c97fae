"""Plain NumPy / Python restatements of the shared device primitives (nyxus_amd/csrc/device_math.h, sort_lds.h): what
tests/cpp/device_prims_probe.hip must return.  No GPU is needed to import this; tests/test_device_prims_cpu.py keeps it honest.

* fast_log2f / plogp: the float32 steps of the reference's fast_log10 (helpers/helpers.h) up to its `lg2`, same order, np.float32.
* the four binning functions: float64, the operation order of the reference (features/texture_feature.h, helpers/helpers.h).
* exact integer models of the 24-bit multiplies, the median clamp, the counting-table word, RowCol, the wave reductions / scans /
  shifts / transposed sums.
* correctly rounded references for a / b, 1 / b (IEEE float64) and 1 / sqrt(x) (mpmath, one rounding), with the error of a result
  expressed as ordinal distance: the count of doubles between it and the correctly rounded value."""
import numpy as np

U32 = np.uint32
MASK32 = 0xFFFFFFFF


# ---- fast_log2f, plogp ------------------------------------------------------------------------------------------------------------
def fast_log2f(x):
    """float32 array: lg2 of helpers.h fast_log10 for float64 input x (any shape)."""
    xf = np.asarray(x, np.float64).astype(np.float32)
    ui = np.ascontiguousarray(xf).view(np.uint32)
    exp_ = ((ui & U32(0x7F800000)) >> U32(23)).astype(np.int32)
    greater = (ui & U32(0x00400000)) != 0
    stuffed = (ui & U32(0x007FFFFF)) | np.where(greater, U32(0x3F000000), U32(0x3F800000)).astype(np.uint32)
    signif = np.ascontiguousarray(stuffed).view(np.float32)
    fexp = exp_.astype(np.float32) - np.where(greater, np.float32(126.0), np.float32(127.0)).astype(np.float32)
    a, b = np.float32(-.6296735), np.float32(1.466967)
    signif = signif - np.float32(1.0)
    t1 = (a * signif) * signif
    t2 = b * signif
    out = (fexp + t1) + t2
    assert out.dtype == np.float32
    return out


def plogp(p, arg):
    """p * float64(fast_log2f(arg + 1e-9)), float64."""
    p, arg = np.asarray(p, np.float64), np.asarray(arg, np.float64)
    return p * fast_log2f(arg + 0.000000001).astype(np.float64)


# ---- binning ------------------------------------------------------------------------------------------------------------------------
def _trunc_u32(v):
    """(uint32) of a float64 that the callers' contract keeps inside [0, 2^32)."""
    return np.asarray(v).astype(np.int64).astype(np.uint32)


def bin_radiomix(x, mn, mx, bin_count):
    x, mn, mx = (np.asarray(v, np.uint32) for v in (x, mn, mx))
    bc = np.asarray(bin_count, np.int64)
    with np.errstate(all="ignore"):
        bin_w = (mx - mn).astype(np.float64) / bc.astype(np.float64)
        yf = (x - mn).astype(np.float64) / bin_w + 1
        yf = np.where(x != 0, yf, 0.0)
        y = _trunc_u32(np.where(np.isfinite(yf), yf, 0.0))
    y = np.minimum(y, bc.astype(np.uint32))
    return np.where(x != 0, y, U32(0)).astype(np.uint32)


def bin_matlab(x, slope, n_levels):
    x = np.asarray(x, np.uint32)
    slope, n = np.asarray(slope, np.float64), np.asarray(n_levels, np.int64).astype(np.uint32)
    scaled_real = np.floor(slope * x.astype(np.float64) + 1.0)
    scaled = _trunc_u32(scaled_real)
    scaled = np.maximum(np.minimum(scaled, n), U32(1))
    return np.where(x == 0, U32(1), scaled).astype(np.uint32)


def matlab_slope(mx, info):
    return np.asarray(info, np.float64) / (np.asarray(mx, np.uint32).astype(np.float64) - 0.)


def bin_pixel(x, mn, mx, info):
    x = np.asarray(x, np.uint32)
    info = np.broadcast_to(np.asarray(info, np.int64), x.shape)
    with np.errstate(all="ignore"):
        rad = bin_radiomix(x, mn, mx, np.where(info < 0, -info, 1))
        mat = bin_matlab(x, np.where(info > 0, matlab_slope(mx, np.where(info > 0, info, 1)), 0.0), np.where(info > 0, info, 1))
    return np.where(info < 0, rad, np.where(info > 0, mat, x)).astype(np.uint32)


def to_grayscale(i, min_i, i_range, n_levels):
    i, min_i, i_range, n_levels = (np.asarray(v, np.uint32) for v in (i, min_i, i_range, n_levels))
    with np.errstate(all="ignore"):
        pi = (i - min_i).astype(np.float64) / i_range.astype(np.float64) * n_levels.astype(np.float64)
    return _trunc_u32(np.where(np.isnan(pi), 0.0, pi))


# ---- exact integer models ---------------------------------------------------------------------------------------------------------------
def _u64(v):
    return np.asarray(v).astype(np.uint64)


def mul24(a, b):
    """low 32 bits of the product of the low 24 bits"""
    return ((_u64(a) & np.uint64(0xFFFFFF)) * (_u64(b) & np.uint64(0xFFFFFF)) & np.uint64(MASK32)).astype(np.uint32)


def mad24(a, b, c):
    return (((_u64(a) & np.uint64(0xFFFFFF)) * (_u64(b) & np.uint64(0xFFFFFF)) + _u64(c)) & np.uint64(MASK32)).astype(np.uint32)


def _sext24(v):
    v = np.asarray(v).astype(np.int64) & 0xFFFFFF
    return np.where(v & 0x800000, v - 0x1000000, v)


def mul_i24(a, b):
    """signed: both factors sign-extended from bit 23; the low 32 bits of the product, as uint32"""
    return ((_sext24(a) * _sext24(b)) & MASK32).astype(np.uint32)


def med3(x, lo, hi):
    return np.sort(np.stack(np.broadcast_arrays(np.asarray(x, np.uint32), U32(lo), U32(hi))), axis=0)[1]


def cnt16_word_offset(ci):
    return ((np.asarray(ci, np.uint32) & U32(0xFFFFFFFE)) << U32(1)).astype(np.uint32)


def rowcol(first, width):
    """(row, col) of a linear index"""
    q, r = np.divmod(np.asarray(first, np.int64), np.asarray(width, np.int64))
    return q, r


def rowcol_walk(first, stride, width, steps):
    """[n][steps + 1][2]: (row, col) of first, first + stride, ... -- the position advances by repeated addition"""
    first, stride, width = (np.asarray(v, np.int64) for v in (first, stride, width))
    out = np.empty((len(first), steps + 1, 2), np.int64)
    p = first.copy()
    for k in range(steps + 1):
        out[:, k, 0], out[:, k, 1] = np.divmod(p, width)
        p = p + stride
    return out


# wave models: v is [..., 64]
def wave_sum(v):
    v = np.asarray(v)
    return np.broadcast_to(v.sum(axis=-1, keepdims=True, dtype=v.dtype), v.shape)


def wave_scan(v):
    v = np.asarray(v)
    return np.cumsum(v, axis=-1, dtype=v.dtype)


def wave_scan_min(v):
    return np.minimum.accumulate(np.asarray(v), axis=-1)


def wave_max(v):
    v = np.asarray(v)
    return np.broadcast_to(v.max(axis=-1, keepdims=True), v.shape)


def row16_sum(v):
    v = np.asarray(v)
    r = v.reshape(v.shape[:-1] + (4, 16))
    return np.broadcast_to(r.sum(axis=-1, keepdims=True, dtype=v.dtype), r.shape).reshape(v.shape)


def row16_max(v):
    v = np.asarray(v)
    r = v.reshape(v.shape[:-1] + (4, 16))
    return np.broadcast_to(r.max(axis=-1, keepdims=True), r.shape).reshape(v.shape)


def lane_plus1(v, fill):
    v = np.asarray(v)
    out = np.empty_like(v)
    out[..., :-1] = v[..., 1:]
    out[..., -1] = fill
    return out


def lane_minus1(v, fill):
    v = np.asarray(v)
    out = np.empty_like(v)
    out[..., 1:] = v[..., :-1]
    out[..., 0] = fill
    return out


def wave_rol1(v):
    return np.roll(np.asarray(v), -1, axis=-1)


def wave_ror1(v):
    return np.roll(np.asarray(v), 1, axis=-1)


def readlane(v, lane):
    v = np.asarray(v)
    return np.broadcast_to(v[..., lane:lane + 1], v.shape)


TRANSPOSE_SHIFT = {4: 4, 8: 3, 16: 2, 64: 0}


def transpose_slot(k):
    """the slot whose wave total lane L returns, for the k-slot transposed sum"""
    lanes = np.arange(64)
    return (lanes >> TRANSPOSE_SHIFT[k]) & (k - 1)


def wave_transpose_sum(v):
    """v: [..., k, 64] -> [..., 64]"""
    v = np.asarray(v)
    k = v.shape[-2]
    tot = v.sum(axis=-1, dtype=v.dtype)                    # [..., k]
    return tot[..., transpose_slot(k)]


# ---- correctly rounded references, ordinal distance ---------------------------------------------------------------------------------------
def ordinal(x):
    """doubles -> int64 that counts them in order (-0.0 and +0.0 share 0)"""
    i = np.ascontiguousarray(np.asarray(x, np.float64)).view(np.int64)
    return np.where(i < 0, -(i & np.int64(0x7FFFFFFFFFFFFFFF)), i)


def ordinal_distance(got, want):
    return np.abs(ordinal(got) - ordinal(want))


def div_exact(a, b):
    return np.asarray(a, np.float64) / np.asarray(b, np.float64)


def rcp_exact(b):
    return 1.0 / np.asarray(b, np.float64)


def rsqrt_mp(x, prec=200):
    """1 / sqrt(x) at `prec` bits, rounded once to double (element by element: for small sets)"""
    import mpmath
    out = np.empty(len(x), np.float64)
    with mpmath.workprec(prec):
        for j, v in enumerate(np.asarray(x, np.float64)):
            out[j] = float(1 / mpmath.sqrt(mpmath.mpf(float(v))))
    return out


def rsqrt_exact(x):
    """Correctly rounded 1 / sqrt(x) for an array.  The bulk goes through np.longdouble (64-bit significand where the platform has
    one); rounding that to double is a second rounding, which can only differ from the single one when the extended value lies within
    its own error of a rounding tie of the doubles -- those elements (a few in a thousand), and everything where longdouble is no
    wider than double, are recomputed with mpmath.  Returns (values, number recomputed)."""
    x = np.asarray(x, np.float64)
    if np.finfo(np.longdouble).nmant < 63:
        return rsqrt_mp(x), len(x)
    xl = x.astype(np.longdouble)
    y = np.longdouble(1) / np.sqrt(xl)
    yd = y.astype(np.float64)
    r = np.abs(y - yd.astype(np.longdouble))                # exact
    h = (np.spacing(np.abs(yd)) / 2).astype(np.longdouble)  # half the gap above yd
    # the extended value errs by at most 1.5 of its ulps (sqrt 1/2, carried through the division, plus the division's own 1/2):
    # below 2^-62 relative; twice that is taken
    tol = np.abs(y) * np.longdouble(2.0 ** -61)
    amb = np.abs(r - h) <= tol
    pow2 = np.frexp(yd)[0] == 0.5                           # below a power of two the gap, and the tie's distance, is half of that
    amb |= pow2 & (np.abs(r - h / 2) <= tol)
    idx = np.flatnonzero(amb)
    if len(idx):
        yd[idx] = rsqrt_mp(x[idx])
    return yd, len(idx)
