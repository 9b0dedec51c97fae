"""Inputs for the kernels' own seams of roi_vol.hip (tests/test_vol_exact_cpu.py, tests/test_vol_exact_gpu.py): seeded ROIs of a few
thousand cells at most unless stated, each group written for one line of the kernel.  tests/vol_cases.py holds the cases recorded from
the reference's classes; nothing here is recorded -- the GLCM groups are held to tests/vol_exact_ref.py, the intensity groups to
vol_ref.intensity_rows and to plain NumPy integers.

GLCM groups (GLCM_CASES: Case(group, name, batch name, settings))
  widths   vol_glcm_kernel's lane-sharing width LW = 8 | 16 | 32 | 64 (switches at w = 8|9, 16|17, 32|33) and the second and third trip of
           the x loop (64|65, 128|129): full and 70 %-filled boxes of w x 3 x 3
  rows     the row loop's stride of 4 * rpw rows: w = 8 (rpw 8) and w = 64 (rpw 1) with h * d just under, at, just over one stride and
           just over two, as h x 1, 1 x d and a proper h x d
  negshift directions with a negative dy or dz: pairs at both borders of the axis (test_vol_exact_cpu asserts it from the matrices)
  tail     the word-wise read of the box: cells % 4 in {0, 1, 2, 3} with the last cell occupied, under matlab binning (the bytes behind
           the box hold level 1, not 0) with and without glcm_symmetric, and in IBSI mode
  levels   the 128-bit presence map and its rank table across plo | phi (levels 64 | 65): explicit intensities, so the level set is known
  offsets  glcm_offset in {1, 2, w - 1, w, w + 1} on a 9x4x3 box, 3 on a box of depth 2 (every dz != 0 direction blank), 300 on a
           310x2x2 box
  needles  65534x1x1, 1x65534x1, 1x1x65534, fully occupied, 6-bit intensities: the coordinate extremes, the global-memory path with one
           row, 65534 rows of one cell
  seam     the LDS-staging seam (32768 cells): vol_cases' seam and blob40 batches, a 33x32x31 box (32736 cells, the nearest below the seam a
           width of 33 reaches) and 64x32x16 (exactly at it)
Intensity groups (one-dimensional clouds: the intensity block needs no boxes)
  sort     n in SORT_N x ranges whose bit count is in SORT_BITS (the pass count of the 4-bit radix sort, and so which of the two buffers ends
           up as the table), each ROI once ascending and once descending; one ROI of 4097 values over the full 32-bit range
  mode     sorted-run layouts the gallop-and-bisect search has to get right (MODE_LAYOUTS)
  bins     grey_depth in {1, -1, 16384, -16384} on three of the sort ROIs (BINS_ROIS); 16385 and -16385 are refused
  chunk    the 12 ROIs of vol_cases' `boxes` tiled to 65535 + 15 ROIs: the bound of a chunk (a grid dimension)
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from nyxus_amd import _abi
from tests import vol_cases
from tests.vol_cases import _blob, _full, _roi

Case = namedtuple("Case", "group name bname mode")
Case.id = property(lambda c: "%s-%s" % (c.group, c.name))

WIDTHS = (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
SORT_N = (1, 2, 255, 256, 257, 511, 512, 513, 767, 1025)
SORT_BITS = (0, 1, 4, 5, 8, 9, 16, 31, 32)
CHUNK_ROIS = 65535 + 15


def lane_width(w: int) -> int:
    """LW of vol_glcm_kernel: the power of two in [8, 64] that covers min(w, 64)."""
    lw = 64
    while lw > 8 and lw // 2 >= w:
        lw //= 2
    return lw


def _full_roi(rng, w, h, d, lo, hi):
    return _blob(rng, w, h, d, 2.0, lo, hi)                # (fill above 1: every cell kept)


def _widths():
    rng = np.random.default_rng(8091617)
    return [f(rng, w, 3, 3, *a) for w in WIDTHS for f, a in ((_full_roi, (1, 4000)), (_blob, (0.7, 1, 4000)))]


def row_boxes():
    """(w, h, d) of the rows group: for each width the products h * d in {4 rpw - 1, 4 rpw, 4 rpw + 1, 8 rpw + 1}, as h x 1, 1 x d and,
    where the product is composite, its most square factorisation."""
    out = []
    for w in (8, 64):
        rpw = 64 // lane_width(w)
        for p in (4 * rpw - 1, 4 * rpw, 4 * rpw + 1, 8 * rpw + 1):
            out += [(w, p, 1), (w, 1, p)]
            f = max(k for k in range(1, int(p ** 0.5) + 1) if p % k == 0)
            if f > 1:
                out.append((w, p // f, f))
    return out


def _rows():
    rng = np.random.default_rng(32641)
    return [_blob(rng, w, h, d, 0.85, 1, 4000) for w, h, d in row_boxes()]


def _negshift():
    rng = np.random.default_rng(1311)
    R = [_blob(rng, 6, 5, 4, 0.7, 1, 4000), _blob(rng, 5, 7, 6, 0.6, 1, 4000), _full_roi(rng, 4, 5, 5, 1, 4000)]
    return R


TAIL_BOXES = ((4, 3, 3), (5, 3, 3), (7, 3, 6), (3, 3, 3), (13, 12, 7), (33, 33, 1), (10, 109, 1), (1091, 1, 1))


def _tail():
    rng = np.random.default_rng(4123)
    # intensities up to 100: the batch also runs in IBSI mode (the levels are the intensities)
    return [_blob(rng, w, h, d, 0.7, 1, 100) for w, h, d in TAIL_BOXES]


def _from_levels(rng, w, h, d, values, zeros=0.1):
    """A full w x h x d box whose intensities are drawn from `values` (every one of them occurs), `zeros` of the cells 0."""
    x, y, z = _full(w, h, d)
    values = np.asarray(values, np.int64)
    v = values[rng.integers(0, len(values), len(x))]
    # neighbouring cells correlate: a ramp of value ranks under the noise, so the matrices are not flat
    ramp = (x + y + z) * len(values) // (w + h + d)
    pick = np.clip(ramp + rng.integers(-2, 3, len(x)), 0, len(values) - 1)
    v = np.where(rng.random(len(x)) < 0.6, values[pick], v)
    v[rng.random(len(x)) < zeros] = 0
    v[rng.permutation(len(x))[:len(values)]] = values      # every value occurs
    return _roi(x, y, z, v.astype(np.uint32), (w, h, d))


def radiomics_value(level: int) -> int:
    """An intensity that radiomics binning with a bin width of 8 from a minimum of 0 puts into `level` (>= 1): the middle of its bin."""
    return (level - 1) * 8 + 4


def _levels(which):
    rng = np.random.default_rng(646566)
    if which == "r66":
        # minimum 0 (a zero voxel has level 0 and is not counted), maximum 66 * 8: bin width 8 at 66 bins, the maximum in the top bin
        r = _from_levels(rng, 9, 6, 5, [radiomics_value(l) for l in (63, 64, 65)] + [66 * 8])
        r["inten"][0] = 0
        return [r]
    if which == "r128":
        a = _from_levels(rng, 9, 6, 5, [radiomics_value(l) for l in (1, 64, 65)] + [128 * 8])
        b = _from_levels(rng, 12, 10, 9, [radiomics_value(l) for l in range(1, 128)] + [128 * 8])
        a["inten"][0] = b["inten"][0] = 0
        return [a, b]
    if which == "ibsi":
        R = [_from_levels(rng, 9, 8, 7, np.arange(1, top + 1)) for top in (64, 65, 128)]
        R.append(_from_levels(rng, 6, 5, 4, [65], zeros=0))
        R[-1]["inten"][rng.random(120) < 0.3] = 0           # the only non-zero level is 65: plo stays empty
        R[-1]["inten"][[0, -1]] = 65
        return R
    if which == "m128":
        return [_blob(rng, 12, 10, 9, 0.8, 1, 4095)]
    raise KeyError(which)


def _offsets(which):
    rng = np.random.default_rng(94312)
    if which == "9x4x3":
        return [_blob(rng, 9, 4, 3, 0.85, 1, 4000)]
    if which == "depth2":
        return [_blob(rng, 7, 6, 2, 0.85, 1, 4000)]
    return [_blob(rng, 310, 2, 2, 0.85, 1, 4000)]


def _needles():
    rng = np.random.default_rng(65534)
    R = []
    for axis in range(3):
        n = 65534
        c = [np.zeros(n, np.int64)] * 3
        c[axis] = np.arange(n)
        # 6-bit values that drift along the needle under noise, squared: neighbours correlate and the distribution is skewed, so that no
        # column is a sum that cancels to nearly nothing
        u = np.arange(n) * 52 // n + rng.integers(0, 12, n)
        v = 1 + u * u // 63
        R.append(_roi(c[0], c[1], c[2], v.astype(np.uint32)))
    return R


def _seam33():
    rng = np.random.default_rng(3332768)
    return [_blob(rng, 33, 32, 31, 0.7, 100, 4095), _blob(rng, 64, 32, 16, 0.7, 0, 4095)]


# ---- intensity groups -------------------------------------------------------------------------------------------------------

def _cloud(v):
    n = len(v)
    return _roi(np.arange(n) % 60000, np.zeros(n, np.int64), np.zeros(n, np.int64), np.asarray(v, np.uint32), (min(n, 60000), 1, 1))


def sort_range(bits: int, k: int) -> int:
    """A range whose bit count 32 - clz(range) is `bits`: alternately the largest and the smallest such range."""
    if bits == 0:
        return 0
    return (1 << bits) - 1 if k % 2 == 0 else 1 << (bits - 1)


def sort_values():
    """The 90 value sets [(n, bits, ascending uint32 array)]: min and max of the range are attained (n = 1 can only have range 0)."""
    rng = np.random.default_rng(2564)
    out = []
    for k, n in enumerate(SORT_N):
        for bits in SORT_BITS:
            rg = sort_range(bits, k) if n > 1 else 0
            lo = 1000 if rg < 2 ** 31 else int(rng.integers(0, 2 ** 32 - rg))
            v = rng.integers(0, rg + 1, n, dtype=np.uint64)
            if n > 1:
                v[0], v[-1] = 0, rg
            out.append((n, bits, np.sort(v + np.uint64(lo)).astype(np.uint32)))
    return out


def _sort():
    R = []
    for n, bits, v in sort_values():
        R += [_cloud(v), _cloud(v[::-1])]                  # ascending, descending
    return R


def _sort4097():
    rng = np.random.default_rng(4097)
    v = rng.integers(0, 2 ** 32, 4097, dtype=np.uint64)
    v[7], v[4000] = 0, 2 ** 32 - 1
    v[100:140] = v[99]                                      # a mode that is not the minimum
    return [_cloud(v)]


def runs(lengths, first_value=10, step=3):
    """The sorted array of runs of the given lengths, run k of value first_value + k * step; (array, head index of every run)."""
    lengths = np.asarray(lengths, np.int64)
    v = np.repeat(first_value + step * np.arange(len(lengths)), lengths)
    return v.astype(np.uint32), np.concatenate([[0], np.cumsum(lengths)[:-1]])


def _mode_layouts():
    """name -> (run lengths, index of the run that is the mode).  Singles (runs of 1) place the heads."""
    L = {}
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257):
        # the longest run in the middle, a run one shorter of a smaller value before it and one after it
        near = max(1, n - 1)
        L["len%d" % n] = ([1] * 37 + [near] + [1] * 5 + [n] + [1] * 3 + [near] + [1] * 20, 37 + 1 + 5 if n > 1 else 0)
    L["ends_at_n"] = ([1] * 300 + [6] + [1] * 40 + [7], 300 + 1 + 40)
    L["starts_at_0"] = ([7] + [1] * 300 + [6] + [1] * 40, 0)
    # ties across waves: the head of the smaller value in a LATER wave's stride than the head of the larger one
    L["tie2"] = ([1] * 200 + [9] + [1] * 51 + [9] + [1] * 30, 200)             # heads 200 (wave 3) and 260 (260 % 256 = 4: wave 0)
    L["tie2_same_trip"] = ([1] * 70 + [9] + [1] * 121 + [9] + [1] * 30, 70)    # heads 70 (wave 1) and 200 (wave 3) of the first trip
    L["tie3"] = ([1] * 130 + [12] + [1] * 120 + [12] + [1] * 60 + [12] + [1] * 10, 130)   # heads 130 (wave 2), 262 (wave 0), 334 (wave 1)
    L["long700"] = ([1] * 100 + [300] + [1] * 9 + [700] + [1] * 50, 110)       # threads start inside the run; one at its head
    L["pow2_1023"] = ([1] * 5 + [1023] + [1024] + [1025] + [1] * 3, 7)
    return L


MODE_LAYOUTS = _mode_layouts()


def _mode():
    rng = np.random.default_rng(30609)
    return [_cloud(rng.permutation(runs(lengths)[0])) for lengths, _ in MODE_LAYOUTS.values()]


BINS_ROIS = (2 * (3 * len(SORT_BITS) + 4), 2 * (6 * len(SORT_BITS) + 6) + 1, 2 * (9 * len(SORT_BITS) + 8))   # n = 256 / 8 bits, 512 / 16 bits descending, 1025 / 32 bits
BINS_DEPTHS = (1, -1, 16384, -16384)
BINS_REFUSED = (16385, -16385)


def _chunk():
    b = vol_cases.batch("boxes")
    idx = np.arange(CHUNK_ROIS) % b.n_roi
    return b.select(idx)


_BUILD = {"widths": _widths, "rows": _rows, "negshift": _negshift, "tail": _tail, "levels_r66": lambda: _levels("r66"), "levels_r128": lambda: _levels("r128"),
          "levels_ibsi": lambda: _levels("ibsi"), "levels_m128": lambda: _levels("m128"), "off_9x4x3": lambda: _offsets("9x4x3"),
          "off_depth2": lambda: _offsets("depth2"), "off_310": lambda: _offsets("310"), "needles": _needles, "seam33": _seam33, "sort": _sort,
          "sort4097": _sort4097, "mode": _mode}


@functools.lru_cache(maxsize=None)
def batch(name: str) -> _abi.HostBatch3D:
    if name in ("seam", "blob40", "boxes"):
        return vol_cases.batch(name)
    if name == "chunk":
        return _chunk()
    return _abi.batch3d_from_rois(_BUILD[name]())


def settings(mode) -> _abi.Settings:
    """`mode`: a key of vol_cases.MODES, or a tuple of (field, value) pairs."""
    if isinstance(mode, str):
        return vol_cases.settings(mode)
    s = _abi.default_settings(64)
    for k, v in mode:
        setattr(s, k, v)
    return s


def _m(**kw):
    return tuple(sorted(kw.items()))


R16, M16, M16S, IBSI = _m(glcm_grey_depth=-16), _m(glcm_grey_depth=16), _m(glcm_grey_depth=16, glcm_symmetric=1), _m(ibsi=1)

GLCM_CASES = (
    [Case("widths", n, "widths", m) for n, m in (("radiomics16", R16), ("matlab16", M16))] +
    [Case("rows", n, "rows", m) for n, m in (("radiomics16", R16), ("matlab16_sym", M16S))] +
    [Case("negshift", "offset%d" % o, "negshift", _m(glcm_grey_depth=-16, glcm_offset=o)) for o in (1, 2)] +
    [Case("tail", n, "tail", m) for n, m in (("matlab16", M16), ("matlab16_sym", M16S), ("ibsi", IBSI))] +
    [Case("levels", "radiomics_63_to_66", "levels_r66", _m(glcm_grey_depth=-66)), Case("levels", "radiomics_128", "levels_r128", _m(glcm_grey_depth=-128)),
     Case("levels", "ibsi_64_65_128", "levels_ibsi", IBSI), Case("levels", "matlab128", "levels_m128", _m(glcm_grey_depth=128))] +
    [Case("offsets", "9x4x3_offset%d" % o, "off_9x4x3", _m(glcm_grey_depth=-16, glcm_offset=o)) for o in (1, 2, 8, 9, 10)] +
    [Case("offsets", "depth2_offset3", "off_depth2", _m(glcm_grey_depth=-16, glcm_offset=3)),
     Case("offsets", "310x2x2_offset300", "off_310", _m(glcm_grey_depth=-16, glcm_offset=300))] +
    [Case("needles", n, "needles", m) for n, m in (("matlab64_sym", _m(glcm_grey_depth=64, glcm_symmetric=1)), ("ibsi", IBSI))] +
    [Case("seam", "seam_r64", "seam", "r64"), Case("seam", "seam_matlab", "seam", "matlab"), Case("seam", "blob40_cap_radiomics", "blob40", "cap_radiomics"),
     Case("seam", "blob40_cap_matlab", "blob40", "cap_matlab"), Case("seam", "w33_r64", "seam33", "r64"), Case("seam", "w33_matlab", "seam33", "matlab")])
GLCM_GROUPS = tuple(dict.fromkeys(c.group for c in GLCM_CASES))
DEVICE_CASE = next(c for c in GLCM_CASES if c.group == "widths" and c.name == "radiomics16")     # the group that also runs from device memory


def of_group(g):
    return [c for c in GLCM_CASES if c.group == g]


@functools.lru_cache(maxsize=None)
def exact(c: Case):
    """The exact rows of a GLCM case (computed once, shared by the tests)."""
    from tests import vol_exact_ref as vx
    return tuple(vx.exact_rows(batch(c.bname), settings(c.mode)))


@functools.lru_cache(maxsize=None)
def reference(c: Case):
    """vol_ref's GLCM block of a case (the log columns are compared with it), read-only."""
    from tests import vol_ref
    T = vol_ref.glcm_rows(batch(c.bname), settings(c.mode))
    T.setflags(write=False)
    return T
