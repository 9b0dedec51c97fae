"""Inputs of the volume tests (tests/test_vol_cpu.py, tests/test_vol_gpu.py) and of tests/golden/vol/make_vol_golden.py: batches of
volumetric ROIs rebuilt from seeds, the settings they run under, and the one rule that takes values out of the comparison with the
reference.  The cases were chosen for the reference's behaviour (blank directions, the binning modes, the level cap, the LDS-staging seam)
and are what is recorded; the kernels' own seams (lane-sharing widths, rows per wave, the presence map, tail words, the chunk bound, the
voxel sort and the mode search) are the cases of tests/vol_edge_cases.py, which are held to exact values and need no recording.

BATCHES
  boxes   1x1x1 (no pair in any direction) | 2x1x1, 1x2x1, 1x1x2 (one direction has pairs) | 2x2x2 full | the slab 7x5x1 (every dz != 0
          direction blank) | 3x3x3 without its centre voxel | 3x3x3 with a zero-intensity voxel inside | an L-shaped cloud in a 4x3x2 box
          (negative dy / dz at both borders) | a flat 3x3x2 patch | an all-zero 2x2x2 patch | a 5x4x3 blob.  Intensities stay below the
          level cap, so the batch also runs in IBSI mode.
  seam    boxes of 32767, 32768 and 32769 cells (one under, at, and one over the LDS-staging seam of the binned box), 12-bit blobs
  blob40  one 40x40x40 blob (the global workspace), 16-bit intensities
  wide    16-bit and 32-bit intensity ranges in 10x9x8 boxes (the intensity block's sort over every digit)
  over    one ROI whose largest intensity is the level cap + 1 (IBSI mode must refuse it)
The empty ROI (no voxels) is appended by the tests that want one (with_empty): the reference is never handed it.
"""
from __future__ import annotations

import numpy as np

from nyxus_amd import _abi

N_INT, N_DIR, N_ANG, N_AVE = 36, 13, 30, 29
N_COL = N_INT + N_ANG * N_DIR + N_AVE
LDS_CELLS = 32768            # kVolLdsCells of roi_vol.h
LEVEL_CAP = _abi.VOL_GLCM_MAX_LEVELS
SHIFTS = [(1, 1, 1), (1, 1, 0), (1, 1, -1), (1, 0, 1), (1, 0, 0), (1, 0, -1), (1, -1, 1), (1, -1, 0), (1, -1, -1), (0, 1, 1), (0, 1, 0), (0, 1, -1),
          (0, 0, 1)]         # (dx, dy, dz)


def _full(w, h, d):
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    return x.ravel(), y.ravel(), z.ravel()


def _roi(x, y, z, v, box=None):
    r = {"x": np.asarray(x), "y": np.asarray(y), "z": np.asarray(z), "inten": np.asarray(v, np.uint32), "origin": (0, 0, 0)}
    r["box"] = box if box is not None else (int(r["x"].max()) + 1, int(r["y"].max()) + 1, int(r["z"].max()) + 1)
    return r


def _blob(rng, w, h, d, fill, lo, hi):
    x, y, z = _full(w, h, d)
    keep = rng.random(len(x)) < fill
    keep[[0, -1]] = True                                   # the cloud spans its box
    # smooth-ish values: a ramp plus noise, so that neighbouring levels repeat
    v = lo + ((x + 2 * y + 3 * z) * (hi - lo) // max(1, (w + 2 * h + 3 * d)) + rng.integers(0, max(2, (hi - lo) // 6), len(x))) % (hi - lo + 1)
    return _roi(x[keep], y[keep], z[keep], v[keep].astype(np.uint32), (w, h, d))


def _boxes():
    rng = np.random.default_rng(20240611)
    R = []
    R.append(_roi([0], [0], [0], [7]))
    R.append(_roi([0, 1], [0, 0], [0, 0], [5, 9]))
    R.append(_roi([0, 0], [0, 1], [0, 0], [4, 4 + 13]))
    R.append(_roi([0, 0], [0, 0], [0, 1], [30, 2]))
    x, y, z = _full(2, 2, 2)
    R.append(_roi(x, y, z, rng.integers(1, 40, 8)))
    x, y, z = _full(7, 5, 1)
    R.append(_roi(x, y, z, rng.integers(1, 25, 35)))
    x, y, z = _full(3, 3, 3)
    keep = ~((x == 1) & (y == 1) & (z == 1))
    R.append(_roi(x[keep], y[keep], z[keep], rng.integers(1, 12, 26), (3, 3, 3)))
    v = rng.integers(1, 12, 27)
    v[13] = 0
    R.append(_roi(x, y, z, v))
    x, y, z = _full(4, 3, 2)
    keep = (z == 0) & ((y == 0) | (x == 0)) | (z == 1) & (x == 3) & (y == 2) | (z == 1) & (x == 0) & (y == 0)
    R.append(_roi(x[keep], y[keep], z[keep], rng.integers(1, 50, int(keep.sum())), (4, 3, 2)))
    x, y, z = _full(3, 3, 2)
    R.append(_roi(x, y, z, np.full(18, 21)))
    x, y, z = _full(2, 2, 2)
    R.append(_roi(x, y, z, np.zeros(8)))
    R.append(_blob(rng, 5, 4, 3, 0.8, 1, 100))
    return R


def _seam():
    rng = np.random.default_rng(77)
    return [_blob(rng, 151, 31, 7, 0.7, 100, 4095), _blob(rng, 32, 32, 32, 0.7, 0, 4095), _blob(rng, 331, 11, 9, 0.7, 1, 4000)]


_CACHE = {}


def batch(name: str) -> _abi.HostBatch3D:
    if name not in _CACHE:
        if name == "boxes":
            R = _boxes()
        elif name == "seam":
            R = _seam()
        elif name == "blob40":
            R = [_blob(np.random.default_rng(4040), 40, 40, 40, 0.6, 300, 65535)]
        elif name == "wide":
            rng = np.random.default_rng(3232)
            a = _blob(rng, 10, 9, 8, 0.9, 0, 65535)
            b = _blob(rng, 10, 9, 8, 0.9, 5, 4294967295)
            b["inten"][:3] = [5, 4294967295, 2147483648]
            c = _blob(rng, 10, 9, 8, 0.9, 1000, 1000 + 70000)
            c["inten"][5:25] = c["inten"][4]                # a mode that is not the minimum
            R = [a, b, c]
        elif name == "over":
            x, y, z = _full(3, 2, 2)
            R = [_roi(x, y, z, np.r_[np.arange(1, 12), LEVEL_CAP + 1])]
        else:
            raise KeyError(name)
        _CACHE[name] = _abi.batch3d_from_rois(R)
    return _CACHE[name]


def with_empty(b: _abi.HostBatch3D, at: int = 1) -> _abi.HostBatch3D:
    """`b` with an ROI of zero voxels (box 2x2x2) inserted at row `at`."""
    off = b.px_offset.astype(np.int64)
    ins = lambda a, v: np.insert(a, at, v)
    return _abi.HostBatch3D(ins(b.roi_label, 999), np.insert(off, at, off[at]).astype(np.uint64), b.x, b.y, b.z, b.inten, ins(b.bbox_w, 2), ins(b.bbox_h, 2),
                            ins(b.bbox_d, 2), ins(b.min_inten, 0), ins(b.max_inten, 0))


MODES = {
    # radiomics binning with fewer distinct levels than bins
    "radiomics": dict(glcm_grey_depth=-20),
    "matlab": dict(glcm_grey_depth=16),
    "matlab_sym": dict(glcm_grey_depth=16, glcm_symmetric=1),
    "ibsi": dict(ibsi=1),
    "offset2": dict(glcm_grey_depth=-20, glcm_offset=2),
    "softnan": dict(glcm_grey_depth=-20, soft_nan=-7.5),
    "cap_matlab": dict(glcm_grey_depth=LEVEL_CAP),
    "cap_radiomics": dict(glcm_grey_depth=-LEVEL_CAP),
    "r64": dict(glcm_grey_depth=-64, grey_depth=100),
}
# (batch, mode) pairs that are recorded
CASES = ([("boxes", m) for m in ("radiomics", "matlab", "matlab_sym", "ibsi", "offset2", "softnan", "cap_matlab", "cap_radiomics")] +
         [("seam", "r64"), ("seam", "matlab"), ("blob40", "cap_radiomics"), ("blob40", "cap_matlab"), ("blob40", "offset2"), ("wide", "r64"),
          ("wide", "matlab")])


def case_name(bname: str, mode: str) -> str:
    return f"{bname}__{mode}"


def settings(mode: str) -> _abi.Settings:
    s = _abi.default_settings(64)
    for k, v in MODES[mode].items():
        setattr(s, k, v)
    return s


def api_volumes():
    """Two volumes [2, 6, 9, 10] of uint16 with three and two labelled ROIs (one of them a single voxel)."""
    rng = np.random.default_rng(606)
    I = rng.integers(0, 3000, (2, 6, 9, 10)).astype(np.uint16)
    M = np.zeros(I.shape, np.uint16)
    M[0, 0:3, 0:4, 0:5] = 3
    M[0, 2:6, 5:9, 4:10] = 1
    M[0, 0, 8, 9] = 7
    M[1, 1:5, 1:8, 2:9] = 2
    M[1, 1:3, 1:3, 2:4] = 5
    return I, M


def rule_excluded(b: _abi.HostBatch3D, s: _abi.Settings) -> np.ndarray:
    """[n_roi x N_COL] True where the reference's result is undefined and the recording therefore holds this package's defined value
    ("Undefined in the reference").  Decided from the inputs alone:
      * an ROI without voxels: every column (the reference is never handed one; the row is soft_nan);
      * a flat ROI (max_inten == min_inten) under radiomics binning of the GLCM block: to_grayscale_radiomix divides by a zero bin
        width and converts the NaN to an integer; the GLCM columns (every level is 0 here: blank directions, soft_nan)."""
    ex = np.zeros((b.n_roi, N_COL), bool)
    ex[b.counts() == 0, :] = True
    if not s.ibsi and s.glcm_grey_depth < 0:
        ex[b.max_inten == b.min_inten, N_INT:] = True
    return ex


def column_names():
    from nyxus_amd import featureset3d as f3
    return f3.INTENSITY_3D + [f"{c}_{k}" for c in f3.GLCM_3D_ANGLED for k in range(N_DIR)] + f3.GLCM_3D_AVE


def compare(got: np.ndarray, want: np.ndarray, names=None):
    """The project's comparison policy (tests/parity.py: integer-valued and order-statistic columns bit for bit -- parity.EXACT_COLUMNS
    behind the "3" --, the rest within parity.REL_TOL) on volume tables.  Returns (mismatches, largest relative difference of the
    intensity block, ... of the GLCM block) over the finite, non-exact entries."""
    from tests import parity
    names = names or column_names()
    base = []
    for n in names:
        n = n[1:]
        if n.startswith("GLCM_INFOMEAS2_") and n.rsplit("_", 1)[1].isdigit():
            n = n.rsplit("_", 1)[0]                        # (the policy's absolute allowance for this column goes by its base name)
        elif n.startswith("GLCM_") and n.rsplit("_", 1)[1].isdigit():
            n = n.rsplit("_", 1)[0] + "_dir" + n.rsplit("_", 1)[1]
        base.append(n)
    bad = parity.compare_tables(got, want, base)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - want) / np.abs(want)
    rel[~np.isfinite(rel)] = 0.0
    rel[(got == want)] = 0.0
    # (values the policy passes on an absolute allowance are rounding noise around 0: no relative figure)
    scale = np.nanmax(np.abs(np.where(np.isfinite(want), want, 0.0)), axis=0, initial=0.0) if len(want) else np.zeros(want.shape[1])
    rel[np.abs(want) <= 1e-9 * scale[None, :]] = 0.0
    im2 = np.array([n in ("GLCM_INFOMEAS2", "GLCM_INFOMEAS2_AVE") for n in base])
    rel[:, im2] = np.where(np.abs(got - want)[:, im2] <= 1e-7, 0.0, rel[:, im2])
    is_int = np.array([n.startswith("3") and not n.startswith("3GLCM_") for n in names])
    return bad, float(rel[:, is_int].max(initial=0.0)), float(rel[:, ~is_int].max(initial=0.0))
