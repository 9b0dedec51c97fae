"""Inputs shared by tests/test_soft_nan_cpu.py and tests/test_soft_nan_gpu.py: ROIs on which the twelve core families are undefined
somewhere (constant and blank ROIs, single pixels, two values only, pairs without a neighbour), run at a soft_nan that is not 0.0 so
that "wrote soft_nan", "wrote a literal zero" and "never wrote the cell" are three different tables."""
import numpy as np

from nyxus_amd import _abi
from tests import synth

SOFT_NAN = -7.5

GLCM = _abi.FAM_GLCM
TEXTURE = _abi.FAM_GLRLM | _abi.FAM_GLSZM | _abi.FAM_NGTDM
DEPENDENCE = _abi.FAM_GLDZM | _abi.FAM_GLDM | _abi.FAM_NGLDM
SHAPE = _abi.FAM_GABOR | _abi.FAM_ZERNIKE
MOMENTS = _abi.FAM_SMOMS | _abi.FAM_IMOMS
INTENSITY = _abi.FAM_INTENSITY


def roi(x, y, inten):
    """ROI dict in the column-major pixel order of the reference's scan (x outer, y inner)."""
    x, y = np.asarray(x, np.int64).ravel(), np.asarray(y, np.int64).ravel()
    v = np.broadcast_to(np.asarray(inten).ravel(), x.shape)
    o = np.lexsort((y, x))
    return dict(x=x[o], y=y[o], inten=v[o].astype(np.uint32))


def box(w, h, values):
    """w x h box; `values` is a scalar or w * h values in row-major order."""
    yy, xx = np.mgrid[0:h, 0:w]
    v = np.broadcast_to(np.asarray(values, np.uint64).ravel(), (w * h,)) if np.ndim(values) else np.full(w * h, values, np.uint64)
    return roi(xx, yy, v)


def disc(cx, cy, r2, w, h):
    """Pixel coordinates (x, y) of (x - cx)^2 + (y - cy)^2 <= r2 inside a w x h box, row-major."""
    yy, xx = np.mgrid[0:h, 0:w]
    m = (xx - cx) ** 2 + (yy - cy) ** 2 <= r2
    return xx[m], yy[m]


def five_kinds(x, y, rng, hi=4096):
    """Constant, blank, two-value, random and one-non-zero-pixel fillings of one pixel set."""
    n = len(x)
    one = np.zeros(n, np.uint32)
    one[n // 2] = 77
    return [roi(x, y, np.full(n, 1234)), roi(x, y, np.zeros(n)), roi(x, y, np.where(np.arange(n) % 2, 3000, 10)),
            roi(x, y, rng.integers(1, hi, n)), roi(x, y, one)]


def degenerate_rois():
    """The 16 hand-made ROIs: every one fits the smallest size class (<= 256 px, sides <= 32) except the 64 x 1 row (index 7)."""
    rng = np.random.default_rng(2)
    rois = [roi([0], [0], [9]),
            roi([0], [0], [0]),
            box(2, 1, [3, 3]),
            box(2, 1, [3, 8]),
            roi([0, 3], [0, 3], [1, 200]),
            box(4, 1, 0),
            box(2, 2, 7),
            box(64, 1, 42),
            box(1, 30, rng.integers(1, 300, 30)),
            box(3, 2, [0, 5, 0, 7, 0, 9]),
            box(2, 2, [2 ** 32 - 1, 2 ** 32 - 2, 1, 2 ** 31])]
    x, y = disc(5, 6, 30, 11, 13)
    return rois + five_kinds(x, y, rng)


ROW64 = 7                           # index of the 64 x 1 row in degenerate_rois(): the one ROI beyond the smallest size class


def random_rois():
    return synth.random_rois(120, seed=11, rmax=14, value_modes=(4096, 256, 8, 3, 2 ** 32 - 1))


def for_ibsi(rois, drop_blank):
    """Intensities mod 9 (few levels under identity binning).  drop_blank: without the ROIs that became all-zero -- the reference
    dereferences an empty set there in IBSI NGTDM (ngtdm.cpp:58)."""
    out = [dict(r, inten=(np.asarray(r["inten"], np.uint64) % 9).astype(np.uint32)) for r in rois]
    return [r for r in out if np.asarray(r["inten"]).max() > 0] if drop_blank else out


def settings(gd, ibsi=False, soft_nan=SOFT_NAN, na=4, offset=1):
    s = _abi.default_settings(gd, ibsi)
    s.soft_nan = soft_nan
    s.glcm_n_angles = na
    s.glcm_offset = offset
    return s


# (name, grey depth, ibsi, GLCM angles, GLCM offset) per family group -- part 1c of the pull request that added this file
GLCM_CONFIGS = [("gd8", 8, False, 4, 1), ("gd64", 64, False, 4, 1), ("gd-16", -16, False, 4, 1), ("gd100_na2", 100, False, 2, 1),
                ("gd20_ibsi", 20, True, 4, 1), ("gd8_off3", 8, False, 4, 3)]
TEX_CONFIGS = [("gd8", 8, False, 4, 1), ("gd64", 64, False, 4, 1), ("gd-16", -16, False, 4, 1), ("gd20_ibsi", 20, True, 4, 1)]
DEP_CONFIGS = [c for c in TEX_CONFIGS if c[1] > 0]          # the dependence families refuse radiomics binning (negative depth)
ONE_CONFIG = [("gd8", 8, False, 4, 1)]

GROUPS = {"glcm": (GLCM, GLCM_CONFIGS), "texture": (TEXTURE, TEX_CONFIGS), "dependence": (DEPENDENCE, DEP_CONFIGS),
          "shape": (SHAPE, TEX_CONFIGS), "moments": (MOMENTS, ONE_CONFIG), "intensity": (INTENSITY, ONE_CONFIG)}


def cases(group, ibsi, which):
    """The ROI list of `which` ("degenerate" / "random") for a family group."""
    rois = degenerate_rois() if which == "degenerate" else random_rois()
    if ibsi:
        rois = for_ibsi(rois, drop_blank=group == "texture")
    return rois


# ---- one size class up: the workgroup kernels -----------------------------------------------------------------------------------------
def workgroup_rois(n_random=4, seed=5, hi=4096):
    """The same kinds beyond the smallest size class: a constant 40 x 1 row, five 20 x 20 boxes, a constant 61 x 61 disc, constant
    70 x 3 and 130 x 3 strips (beyond one and two wave widths), and a few ordinary companions."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:20, 0:20]
    rois = [box(40, 1, 5)] + five_kinds(xx.ravel(), yy.ravel(), rng, hi)
    rois += [roi(*disc(30, 30, 900, 61, 61), 321), box(70, 3, 11), box(130, 3, 11)]
    comp = [r for r in synth.random_rois(40, seed=seed, rmax=24, value_modes=(hi, 256, 8)) if len(r["x"]) > 300][:n_random]
    assert len(comp) == n_random
    return rois + [dict(x=r["x"], y=r["y"], inten=r["inten"]) for r in comp]


N_WORKGROUP_DEGENERATE = 9          # the hand-made head of workgroup_rois()


def eight_wave_companion(seed=6, hi=4096):
    """A 50 x 48 box of random values: a box >= 48 x 48 makes the 16-bit-matrix launch take eight waves."""
    return box(50, 48, np.random.default_rng(seed).integers(1, hi, 50 * 48))


def wide_range_companion(seed=7):
    x, y = disc(12, 12, 144, 25, 25)
    return roi(x, y, np.random.default_rng(seed).integers(1, 200000, len(x)))


def two_value_extremes():
    x, y = disc(10, 10, 100, 21, 21)
    return roi(x, y, np.where(np.arange(len(x)) % 2, 2 ** 32 - 1, 1))


def beyond_lds_rois(seed=8):
    """Constant, blank, two-value and one-non-zero-pixel 300 x 280 boxes (their planes do not fit LDS) beside three small ROIs.  The
    last box is the one whose co-occurrence matrices are blank: every pair has a zero member."""
    n = 300 * 280
    one = np.zeros(n, np.uint32)
    one[n // 2 + 17] = 77
    small = [r for r in synth.random_rois(12, seed=seed, rmax=10, value_modes=(4096, 256)) if len(r["x"]) > 20][:3]
    return [box(300, 280, 1234), small[0], box(300, 280, 0), small[1], box(300, 280, np.where(np.arange(n) % 2, 3000, 10)), small[2],
            box(300, 280, one)]


BEYOND_LDS_BOXES = [0, 2, 4, 6]     # the rows of the 300 x 280 boxes in beyond_lds_rois()
