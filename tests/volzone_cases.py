"""Inputs of the volume zone tests (tests/test_volzone_cpu.py, tests/test_volzone_gpu.py) and of
tests/golden/volzone/make_volzone_golden.py: batches of volumetric ROIs rebuilt from seeds, the settings the two classes read, and the
one rule that takes values out of the comparison with the reference.  Everything here is recorded from the reference's own classes; the
kernels' seams (the cell range of a workgroup, the lane split of the closing, the dense-table bound) are the cases of
tests/volzone_edge_cases.py, which are held to tests/volzone_ref.py and need no recording.

BATCHES
  boxes   the boxes of tests/vol_cases.py (1x1x1, 2x1x1, 1x2x1, 1x1x2, 2x2x2, 7x5x1, two 3x3x3, an L in 4x3x2, a flat 3x3x2, an all-zero
          2x2x2, a 5x4x3 blob), a third flat ROI (one voxel value over a sparse cloud) and random blobs of 6x7x5, 9x12x10 and 12x12x12
          with few levels, so that runs and zones of many sizes occur.  Intensities stay below the level cap: the batch runs unbinned too.
  conn    connectivity (CONN_PAIRS says what the first four hold): two equal voxels in contact at a corner, an edge and a face; equal levels with
          one background cell between them; an ROI voxel at the background level of matlab binning; the 12^3 two-level checkerboard
          (x + y + z) & 1, exactly 2 zones under 26-connectivity; the 12^3 pattern 1 + (x & 1) + 2 (y & 1) + 4 (z & 1), all singletons.
  runs    5x4x3 boxes: for each of the 13 directions a full-length run through the box (for a direction with a negative component it
          starts at the far face), one broken in the middle, and one that ends at a face.
  snakes  union-find adversaries: a one-voxel-wide serpentine that fills 16^3 (long label chains), a comb, and two spirals of one
          level that meet at a single corner contact in the last slice.
  rule    what volzone_cases.rule_excluded names: a 36x36x37 box with one zone above 46340 cells, a 1x1x600 needle with a run of 520
          cells at level 128 (128 x 512 = 2^16), beside four small blobs.
"""
from __future__ import annotations

import numpy as np

from nyxus_amd import _abi
from tests import vol_cases
from tests.vol_cases import api_volumes, with_empty  # noqa: F401
from tests.volzone_ref import N_CODES, N_COL, N_DIR, N_GLRLM, N_GLSZM, SHIFTS13  # noqa: F401

LEVEL_CAP = _abi.VOLZONE_MAX_LEVELS
W = 4096                     # kVzCellsPerWg of roi_volzone.h: the cells of an ROI's box one workgroup of a sweep owns
DENSE_SIZES = 32             # kVzDenseSizes: zones above it go through the sorted list
SHORT_RUNS = 8               # kVzShortRuns: runs above it are counted in the global table directly
LANES = 64                   # the closing splits run lengths (and list entries) over the lanes of a wave

# mode -> (fields of nyxhip_settings, fields of nyxhip_volzone_settings)
MODES = {
    "radiomics": (dict(), dict(glrlm_grey_depth=-20, glszm_grey_depth=-20)),
    "matlab": (dict(), dict(glrlm_grey_depth=16, glszm_grey_depth=16)),
    "ibsi": (dict(ibsi=1), dict(glrlm_grey_depth=-20, glszm_grey_depth=16)),   # the depths are not read
    "none": (dict(), dict(glrlm_grey_depth=0, glszm_grey_depth=0)),
    "softnan": (dict(soft_nan=-7.5), dict(glrlm_grey_depth=-20, glszm_grey_depth=-20)),
    # both depths at the cap, one matlab and one radiomics: two binned boxes
    "cap": (dict(), dict(glrlm_grey_depth=LEVEL_CAP, glszm_grey_depth=-LEVEL_CAP)),
    "mixed": (dict(), dict(glrlm_grey_depth=-8, glszm_grey_depth=6)),
    "mat4": (dict(), dict(glrlm_grey_depth=4, glszm_grey_depth=4)),
}
CASES = ([("boxes", m) for m in ("radiomics", "matlab", "ibsi", "none", "softnan", "cap", "mixed")] +
         [("conn", "none"), ("conn", "mat4"), ("runs", "none"), ("runs", "matlab"), ("snakes", "none"), ("snakes", "mixed"), ("rule", "none"), ("rule", "ibsi")])


def case_name(bname: str, mode: str) -> str:
    return f"{bname}__{mode}"


def settings(mode: str):
    s = _abi.default_settings(64)
    for k, v in MODES[mode][0].items():
        setattr(s, k, v)
    return s, _abi.VolZoneSettings(**MODES[mode][1])


def roi_from_cube(V: np.ndarray, keep: np.ndarray = None):
    """An ROI whose cloud is the cells of V[z, y, x] where `keep` (default: all), with their values; the box is V's."""
    d, h, w = V.shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    k = np.ones(V.shape, bool) if keep is None else keep
    return {"x": x[k], "y": y[k], "z": z[k], "inten": V[k].astype(np.uint32), "origin": (0, 0, 0), "box": (w, h, d)}


def _few_levels(rng, w, h, d, levels, fill=0.9):
    V = rng.integers(1, levels + 1, (d, h, w))
    V[rng.random(V.shape) < 0.03] = 0                      # zero-intensity voxels inside the cloud
    keep = rng.random(V.shape) < fill
    keep.flat[0] = keep.flat[-1] = True
    V.flat[0], V.flat[-1] = 1, levels
    return roi_from_cube(V, keep)


def _boxes():
    rng = np.random.default_rng(20250301)
    R = vol_cases._boxes()
    V = np.full((3, 4, 5), 9)
    R.append(roi_from_cube(V, rng.random(V.shape) < 0.5))  # a third flat ROI
    R += [_few_levels(rng, 6, 7, 5, 3), _few_levels(rng, 9, 12, 10, 5, 0.8), _few_levels(rng, 12, 12, 12, 2, 0.95), _few_levels(rng, 11, 3, 12, 100)]
    return R


# the first four ROIs of "conn" hold two voxels of level 7: (zones of level 7, runs of level 7 along direction 0) with no binning
CONN_PAIRS = [(1, 1), (1, 2), (1, 2), (2, 2)]


def _conn():
    def two(p, q, box, gap=None):
        V = np.zeros(box[::-1], np.int64)
        V[p[::-1]] = V[q[::-1]] = 7
        keep = V > 0
        if gap is not None:
            V[gap[::-1]] = 3
            keep[gap[::-1]] = True
        else:                                              # a second level keeps the ROI from being flat
            far = (box[0] - 1, 0, 0)
            if V[far[::-1]] == 0:
                V[far[::-1]] = 3
                keep[far[::-1]] = True
        return roi_from_cube(V, keep)
    R = [two((0, 0, 0), (1, 1, 1), (3, 2, 2)),             # corner contact: one zone, one run along (1, 1, 1) only
         two((0, 0, 0), (1, 1, 0), (3, 2, 2)),             # edge contact
         two((0, 0, 0), (0, 1, 0), (3, 2, 2)),             # face contact
         two((0, 0, 0), (2, 0, 0), (3, 1, 1), gap=(1, 0, 0))]     # 7 3 7: two zones of level 7 -- and one of level 3
    # an ROI voxel at the background level of matlab binning: value 0 bins to 1, like the cells outside the cloud
    V = np.array([[[0, 40, 40], [40, 0, 20]], [[20, 20, 0], [0, 40, 0]]])
    keep = np.ones(V.shape, bool)
    keep[1, 1, 2] = False
    R.append(roi_from_cube(V, keep))
    z, y, x = np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij")
    R.append(roi_from_cube(1 + ((x + y + z) & 1)))
    R.append(roi_from_cube(1 + (x & 1) + 2 * (y & 1) + 4 * (z & 1)))
    return R


def _runs():
    R = []
    w, h, d = 5, 4, 3
    for dz, dy, dx in SHIFTS13:
        L = min(n for c, n in zip((dz, dy, dx), (d, h, w)) if c)
        start = (0 if dz >= 0 else d - 1, 0 if dy >= 0 else h - 1, 0 if dx >= 0 else w - 1)
        for kind in ("full", "broken", "face"):
            V = np.full((d, h, w), 2)
            cells = [(start[0] + k * dz, start[1] + k * dy, start[2] + k * dx) for k in range(L)]
            if kind == "face":                             # starts one step in: it ends at the far face
                cells = cells[1:]
            for c in cells:
                V[c] = 9
            if kind == "broken" and L > 2:
                V[cells[L // 2]] = 4
            V[0, 0, 0] = V[0, 0, 0] if (0, 0, 0) in cells else 1
            R.append(roi_from_cube(V))
    return R


def serpentine(n: int) -> np.ndarray:
    """V[z, y, x]: a one-voxel-wide path of level 5 that fills every second row of every second slice of an n^3 box and is joined at
    alternating ends, the rest level 2."""
    V = np.full((n, n, n), 2)
    for z in range(0, n, 2):
        for y in range(0, n, 2):
            V[z, y, :] = 5
            if y + 2 < n:
                V[z, y + 1, (n - 1) if (y // 2) % 2 == 0 else 0] = 5
        if z + 2 < n:
            V[z + 1, 0, 0] = 5                             # one cell joins a slice to the next but one
    return V


def _snakes():
    R = [roi_from_cube(serpentine(16))]
    V = np.full((6, 9, 17), 1)                             # a comb: a spine along x at y = 0, teeth along y at every second x
    V[:, 0, :] = 6
    V[:, :, ::2] = 6
    V[::2, 1:, :] = np.where(V[::2, 1:, :] == 6, 6, 3)
    R.append(roi_from_cube(V))
    V = np.full((4, 9, 9), 1)                              # two arms of level 8 that touch only at a corner in the last slice
    V[:, 0, :4] = 8
    V[:, :4, 0] = 8
    V[:, 8, 5:] = 8
    V[:, 5:, 8] = 8
    V[3, 3, 3] = V[3, 4, 4] = V[3, 5, 5] = 8               # a diagonal bridge in the last slice: corner contacts
    V[3, 1, 1] = V[3, 2, 2] = 8
    V[3, 6, 6] = V[3, 7, 7] = 8
    R.append(roi_from_cube(V))
    return R


def _rule():
    rng = np.random.default_rng(46340)
    V = np.full((37, 36, 36), 5)
    V[rng.random(V.shape) < 0.002] = 9
    V[0, 0, 0] = 1
    assert (V == 5).sum() > 46340
    N = np.full((1, 1, 600), 3)
    N[0, 0, 40:560] = LEVEL_CAP
    N[0, 0, 570:580] = 77
    return [roi_from_cube(V), roi_from_cube(N)] + [_few_levels(rng, 5, 6, 4, 4) for _ in range(4)]


_CACHE = {}


def batch(name: str) -> _abi.HostBatch3D:
    if name not in _CACHE:
        _CACHE[name] = _abi.batch3d_from_rois({"boxes": _boxes, "conn": _conn, "runs": _runs, "snakes": _snakes, "rule": _rule}[name]())
    return _CACHE[name]


def column_names():
    from nyxus_amd import featureset3d as f3
    return [f"{c}_{k}" for c in f3.GLRLM_3D_ANGLED for k in range(N_DIR)] + f3.GLRLM_3D_AVE + f3.GLSZM_3D


def _cols(codes_rl=(), codes_sz=()):
    """the table columns of the named angled GLRLM codes (13 directions and the _AVE column each) and GLSZM codes"""
    from nyxus_amd import featureset3d as f3
    out = []
    for c in codes_rl:
        q = f3.GLRLM_3D_ANGLED.index("3GLRLM_" + c)
        out += list(range(q * N_DIR, (q + 1) * N_DIR)) + [N_CODES * N_DIR + q]
    out += [N_GLRLM + f3.GLSZM_3D.index("3GLSZM_" + c) for c in codes_sz]
    return out


def rule_excluded(b: _abi.HostBatch3D, s: _abi.Settings, t: _abi.VolZoneSettings) -> np.ndarray:
    """[n_roi x N_COL] True where the reference's result is undefined and the recording therefore holds this package's defined value
    ("Undefined in the reference").  Decided from the inputs alone, conservatively -- by the box, never by the runs or
    zones it turns out to hold:
      * an ROI without voxels: every column (the reference is never handed one; the row is soft_nan);
      * double(j * j) with int j overflows above 46340: 3GLRLM_SRE, _LRE, _SRHGLE, _LRLGLE where the largest box side exceeds 46340 (no
        run is longer than a side), 3GLSZM_SAE and _LAE where the box has more than 46340 cells (no zone is larger than the box);
      * inten * inten * j * j is a 32-bit unsigned product: 3GLRLM_SRLGLE and _LRHGLE where (largest possible level) x (largest box
        side) reaches 2^16 -- the largest possible level is |glrlm_grey_depth|, or max_inten when nothing is binned.
    A flat ROI is soft_nan in the reference before any of this is computed: nothing of it is excluded."""
    ex = np.zeros((b.n_roi, N_COL), bool)
    ex[b.counts() == 0, :] = True
    g_rl = 0 if s.ibsi else int(t.glrlm_grey_depth)
    for r in range(b.n_roi):
        if b.counts()[r] == 0 or b.max_inten[r] == b.min_inten[r]:
            continue
        side = int(max(b.bbox_w[r], b.bbox_h[r], b.bbox_d[r]))
        cells = int(b.bbox_w[r]) * int(b.bbox_h[r]) * int(b.bbox_d[r])
        top = abs(g_rl) if g_rl else int(b.max_inten[r])
        if side > 46340:
            ex[r, _cols(("SRE", "LRE", "SRHGLE", "LRLGLE"))] = True
        if top * side >= 1 << 16:
            ex[r, _cols(("SRLGLE", "LRHGLE"))] = True
        if cells > 46340:
            ex[r, _cols((), ("SAE", "LAE"))] = True
    return ex


VARIANCE_COLUMNS = ("GLV", "RV", "ZV")


def floor(names=None) -> np.ndarray:
    """1 for the variance columns (GLV, RV, ZV and their _AVE / directional forms), 0 elsewhere: where all the mass sits on one level or
    one length the exact variance is 0 and either side may land on rounding noise of the mean, so their difference is measured against
    max(|value|, 1), as test_voltex_gpu.FLOOR does."""
    out = []
    for n in (names or column_names()):
        parts = n.split("_")
        out.append(1.0 if parts[1] in VARIANCE_COLUMNS else 0.0)
    return np.array(out)


def rel_diff(got: np.ndarray, want: np.ndarray, names=None) -> np.ndarray:
    """elementwise |got - want| / max(|want|, floor); 0 where both are the same non-finite value; inf where the kinds differ"""
    F = floor(names)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - want) / np.maximum(np.abs(want), F)
    rel = np.where(got == want, 0.0, rel)
    same_kind = (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want)))
    rel = np.where(same_kind, 0.0, rel)
    return np.where(np.isfinite(got) != np.isfinite(want), np.inf, np.where(np.isnan(rel), np.inf, rel))


def compare(got: np.ndarray, want: np.ndarray, names=None):
    """The project's comparison policy (tests/parity.py; none of these columns is integer-exact) on zone tables, with the variance
    columns measured against max(|value|, 1).  Returns (mismatches, largest relative difference)."""
    from tests import parity
    names = names or column_names()
    rel = rel_diff(got, want, names)
    bad = [f"row {r} {names[c]}: got {got[r, c]!r} want {want[r, c]!r}" for r, c in np.argwhere(rel > parity.REL_TOL)]
    return bad, float(rel.max(initial=0.0))


# the metaparameters of the API fixture (Nyxus3DZones.set_metaparam)
API_METAPARAMS = ["3glrlm/greydepth=-24", "3glszm/greydepth=12", "3gldm/greydepth=64", "3ngtdm/greydepth=-32", "3ngtdm/radius=1"]
