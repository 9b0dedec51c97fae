"""Inputs of the volume distance-zone tests (tests/test_voldzone_cpu.py, tests/test_voldzone_gpu.py) and of
tests/golden/voldzone/make_voldzone_golden.py: batches of volumetric ROIs rebuilt from seeds, the settings the class reads, and the one
rule that takes ROIs out of the comparison with the reference.  The kernels' seams (the cell range of a workgroup, the lane split of the
closing, the LDS bound of the emit step) are the cases of tests/voldzone_edge_cases.py, which are held to tests/voldzone_ref.py and need
no recording.

BATCHES
  boxes   the boxes of tests/volzone_cases.py (tiny boxes, flat ROIs, sparse clouds with zero-intensity voxels, blobs of few levels).
          Recorded where the reference is defined on sparse clouds: matlab binning, IBSI mode, no binning.
  full    full boxes without a zero voxel, 1x1x1 .. 13x11x6, few and many levels, a flat one: no level-0 cell under any binning, so the
          batch is recorded under radiomics binning too, and at the level cap.
  conn    what the class's quirks turn on (CONN says which ROI is which): two arms of one level that touch only diagonally; holes one
          cell from a face and at the centre of a plane; a 9 x 9 x 3 full box; a blob for matlab binning, whose background forms zones.
  rule    what voldzone_cases.rule_excluded names: radiomics binning on boxes with holes (cells outside the cloud, voxels of intensity
          0).  Recorded from the restatement alone: the reference's code writes outside its matrix there and is never run on it.
"""
from __future__ import annotations

import numpy as np

from nyxus_amd import _abi
from tests import volzone_cases
from tests.vol_cases import api_volumes, with_empty  # noqa: F401
from tests.volzone_cases import roi_from_cube
from tests.voldzone_ref import N_COL, NAMES  # noqa: F401

LEVEL_CAP = _abi.VOLDZONE_MAX_LEVELS
W = 4096                     # kVzCellsPerWg of roi_volzone.h: the cells of an ROI's box one workgroup of a sweep owns
SHORT_DIST = 8               # kVdzShortDist of roi_voldzone.h: zones of a larger metric are counted in the global table directly
LANES = 64                   # the closing splits the distances over the lanes of a wave

# mode -> fields of nyxhip_settings (default: grey_depth 64)
MODES = {
    "radiomics": dict(grey_depth=-20),
    "matlab": dict(grey_depth=16),
    "ibsi": dict(ibsi=1, grey_depth=-20),                  # the depth is not read
    "none": dict(grey_depth=0),
    "softnan": dict(grey_depth=-20, soft_nan=-7.5),
    "cap": dict(grey_depth=LEVEL_CAP),
    "capneg": dict(grey_depth=-LEVEL_CAP),
    "mat4": dict(grey_depth=4),
}
# recorded from the reference's own class
CASES = ([("boxes", m) for m in ("matlab", "ibsi", "none", "cap")] + [("full", m) for m in ("radiomics", "matlab", "ibsi", "none", "softnan", "cap", "capneg")] +
         [("conn", "ibsi"), ("conn", "none"), ("conn", "mat4")])
# recorded from the restatement alone (every ROI that is not flat is rule-excluded)
RULE_CASES = [("rule", "radiomics"), ("rule", "softnan")]


def case_name(bname: str, mode: str) -> str:
    return f"{bname}__{mode}"


def settings(mode: str) -> _abi.Settings:
    s = _abi.default_settings(64)
    for k, v in MODES[mode].items():
        setattr(s, k, v)
    return s


def _full(rng, w, h, d, levels):
    V = rng.integers(1, levels + 1, (d, h, w))
    V.flat[0], V.flat[-1] = 1, levels
    return roi_from_cube(V)


def _full_boxes():
    rng = np.random.default_rng(20250401)
    R = [_full(rng, *g, levels=lv) for g, lv in (((2, 1, 1), 2), ((1, 2, 1), 2), ((1, 1, 2), 2), ((2, 2, 2), 3), ((7, 5, 1), 3), ((3, 3, 3), 2), ((6, 7, 5), 3),
                                                 ((9, 12, 4), 5), ((13, 11, 6), 2), ((11, 3, 12), 100), ((12, 12, 3), 4))]
    R.append(roi_from_cube(np.full((3, 4, 5), 9)))         # a flat ROI
    R.append(roi_from_cube(np.full((1, 1, 1), 4)))         # a single voxel (flat)
    return R


# the ROIs of "conn"
CONN = {"arms": 0, "hole_near_face": 1, "hole_centre": 2, "slab": 3, "blob": 4}


def _conn():
    rng = np.random.default_rng(20250402)
    A = np.full((2, 6, 6), 1)                              # two arms of level 8 that touch only diagonally: (x 2, y 2) and (x 3, y 3)
    A[:, 2, 0:3] = 8
    A[:, 3, 3:6] = 8
    H1 = np.full((1, 7, 7), 5)                             # a hole at x == 1: one cell from the face
    H1[0, 0, :] = 3
    keep1 = np.ones(H1.shape, bool)
    keep1[0, 3, 1] = False
    H2 = np.full((2, 7, 7), 5)                             # a hole at the centre of the first plane, a zero voxel at that of the second
    H2[:, 6, :] = 3
    keep2 = np.ones(H2.shape, bool)
    keep2[0, 3, 3] = False
    H2[1, 3, 3] = 0
    S = rng.integers(1, 3, (3, 9, 9))                      # 9 x 9 x 3, full
    z, y, x = np.meshgrid(np.arange(6), np.arange(9), np.arange(10), indexing="ij")
    B = 10 + (x + 2 * y + 3 * z) * 2 + rng.integers(0, 30, x.shape)             # (below the level cap: the batch runs unbinned too)
    inside = ((2 * x - 9) / 10.0) ** 2 + ((2 * y - 8) / 9.0) ** 2 + ((2 * z - 5) / 6.0) ** 2 <= 1.0
    return [roi_from_cube(A), roi_from_cube(H1, keep1), roi_from_cube(H2, keep2), roi_from_cube(S), roi_from_cube(B, inside)]


def _rule():
    rng = np.random.default_rng(20250403)
    R = [volzone_cases._few_levels(rng, 6, 7, 5, 3), volzone_cases._few_levels(rng, 9, 12, 10, 5, 0.8), volzone_cases._few_levels(rng, 12, 12, 12, 2, 0.95)]
    V = rng.integers(1, 4, (4, 8, 8)) * 100                # a full box with zero voxels only
    V[rng.random(V.shape) < 0.1] = 0
    V.flat[0] = 100
    R.append(roi_from_cube(V))
    R.append(roi_from_cube(np.full((2, 3, 3), 7), rng.random((2, 3, 3)) < 0.7))   # flat over a sparse cloud: soft_nan, nothing excluded
    return R


_CACHE = {}


def batch(name: str) -> _abi.HostBatch3D:
    if name not in _CACHE:
        _CACHE[name] = _abi.batch3d_from_rois({"boxes": volzone_cases._boxes, "full": _full_boxes, "conn": _conn, "rule": _rule}[name]())
    return _CACHE[name]


def column_names():
    from nyxus_amd import featureset3d as f3
    return list(f3.GLDZM_3D)


def rule_excluded(b: _abi.HostBatch3D, s: _abi.Settings) -> np.ndarray:
    """[n_roi] True where the reference's result is undefined and a recording therefore holds this package's defined value (DESIGN.md
    4.5m).  Decided from the inputs and the settings alone:
      * an ROI without voxels (the reference is never handed one; the row is soft_nan);
      * outside IBSI mode, under radiomics binning (grey_depth < 0), an ROI whose box holds a level-0 cell: a cell outside the cloud
        (fewer voxels than cells) or a voxel of intensity 0 (to_grayscale_radiomix maps 0 to 0 and nothing else).  The reference looks
        the level-0 zone up in a list that has no 0 and writes at row Ng, outside its matrix.
    A flat ROI is soft_nan in the reference before any of this is computed: it is not excluded."""
    ex = b.counts() == 0
    if s.ibsi or s.grey_depth >= 0:
        return ex
    off = b.px_offset.astype(np.int64)
    for r in range(b.n_roi):
        if ex[r] or b.max_inten[r] == b.min_inten[r]:
            continue
        cells = int(b.bbox_w[r]) * int(b.bbox_h[r]) * int(b.bbox_d[r])
        ex[r] = (off[r + 1] - off[r]) < cells or bool((b.inten[off[r]:off[r + 1]] == 0).any())
    return ex


VARIANCE_COLUMNS = ("GLV", "ZDV")


def floor(names=None) -> np.ndarray:
    """1 for the variance columns (GLV, ZDV), 0 elsewhere: where all the mass sits on one level or one distance the exact variance is 0
    and either side may land on rounding noise of the mean, so their difference is measured against max(|value|, 1), as
    volzone_cases.floor does."""
    return np.array([1.0 if n.split("_")[1] in VARIANCE_COLUMNS else 0.0 for n in (names or column_names())])


def rel_diff(got: np.ndarray, want: np.ndarray, names=None) -> np.ndarray:
    """elementwise |got - want| / max(|want|, floor); 0 where both are the same non-finite value; inf where the kinds differ"""
    F = floor(names)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - want) / np.maximum(np.abs(want), F)
    rel = np.where(got == want, 0.0, rel)
    same_kind = (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want)))
    rel = np.where(same_kind, 0.0, rel)
    return np.where(np.isfinite(got) != np.isfinite(want), np.inf, np.where(np.isnan(rel), np.inf, rel))


def compare(got: np.ndarray, want: np.ndarray, names=None, tol=None):
    """The project's comparison policy (tests/parity.py; none of these columns is integer-exact), the variance columns measured against
    max(|value|, 1).  Returns (mismatches, largest relative difference)."""
    from tests import parity
    names = names or column_names()
    rel = rel_diff(got, want, names)
    bad = [f"row {r} {names[c]}: got {got[r, c]!r} want {want[r, c]!r}" for r, c in np.argwhere(rel > (parity.REL_TOL if tol is None else tol))]
    return bad, float(rel.max(initial=0.0))
