"""Edge cases of the volume zone kernels (roi_volzone.hip), rebuilt from seeds and held to tests/volzone_ref.py (no recording).  For every
constant at which a kernel changes form, an ROI one under, at and one over it:

  the cell range of one workgroup   W = kVzCellsPerWg = 4096 cells of the ROI's own box: boxes of W - 1, W and W + 1 cells (one
                                    workgroup | one | two), 2W - 1 (a prime: a needle), 2W and 2W + 2 cells (two | two | three) and
                                    3W + 2 cells (four).  Two or three levels of noise make runs and zones that span the range
                                    boundaries, and the first cell of every range and one of its raster-earlier neighbours
                                    (earlier_neighbour: it lies in the range before) are set to one level inside the cloud, so a run and
                                    a zone cross every boundary.
  the lanes of the closing          the GLRLM closing gives run length j to lane (j - 1) % 64, the GLSZM closing list entry e to lane
                                    e % 64: needles whose longest run (and largest zone) is 63, 64 and 65 cells; slabs with 63, 64 and
                                    65 zones of 34 cells in the list.
  the short-run table               runs of up to kVzShortRuns = 8 cells are counted in LDS: runs of 7, 8 and 9 cells.
  the dense zone table              zones of up to kVzDenseSizes = 32 cells are counted in a table, larger ones are listed and sorted:
                                    zones of 31, 32 and 33 cells.

Each case is (name, batch, settings, zone settings)."""
from __future__ import annotations

import numpy as np

from nyxus_amd import _abi
from tests.volzone_cases import DENSE_SIZES, LANES, SHORT_RUNS, W, roi_from_cube

CELLS_PER_WG = W
WG_BOXES = [(21, 15, 13), (16, 16, 16), (241, 17, 1), (8191, 1, 1), (32, 16, 16), (241, 17, 2), (1229, 5, 2)]   # (w, h, d)
WG_CELLS = [W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 2, 3 * W + 2]


def earlier_neighbour(c, w, h, d):
    """the flat index of a 26-neighbour of cell c that comes before it in raster order: the cell to the left, else the one above, else the
    one in the slice below"""
    z, y, x = c // (w * h), c // w % h, c % w
    return c - 1 if x > 0 else c - w if y > 0 else c - w * h


def _noise(rng, w, h, d, levels, fill=0.9):
    V = rng.integers(1, levels + 1, (d, h, w)) * 9
    keep = rng.random(V.shape) < fill
    keep.flat[0] = keep.flat[-1] = True
    V.flat[0], V.flat[-1] = 9, 9 * levels
    for c in range(W, V.size, W):                          # a pair of one level across every range boundary, inside the cloud
        for q in (c, earlier_neighbour(c, w, h, d)):
            V.flat[q] = 9
            keep.flat[q] = True
    return roi_from_cube(V, keep)


def _needle(lengths, axis):
    """a 1 x 1 x N line of segments of the given lengths at alternating levels along `axis` (0 z, 1 y, 2 x)"""
    v = np.concatenate([np.full(n, 5 + 20 * (k & 1)) for k, n in enumerate(lengths)])
    shape = [1, 1, 1]
    shape[axis] = len(v)
    return roi_from_cube(v.reshape(shape))


def _rows(n_rows, w=DENSE_SIZES + 2):
    """n_rows rows of w cells, row y at level 2 + (y & 1): every row is a zone of its own"""
    V = np.repeat((2 + (np.arange(n_rows) & 1))[:, None], w, axis=1)[None]
    return roi_from_cube(V)


def _settings(kind, soft_nan=0.0):
    s = _abi.default_settings(32)
    s.soft_nan = soft_nan
    if kind == "radiomics":
        return s, _abi.VolZoneSettings(-32, -32)
    if kind == "matlab":
        return s, _abi.VolZoneSettings(16, 16)
    if kind == "mixed":                                    # two binned boxes
        return s, _abi.VolZoneSettings(-24, 12)
    if kind == "none":
        return s, _abi.VolZoneSettings(0, 0)
    s.ibsi = 1
    return s, _abi.VolZoneSettings(0, 0)


_CACHE = {}


def cases():
    if "c" not in _CACHE:
        rng = np.random.default_rng(20250302)
        assert [w * h * d for w, h, d in WG_BOXES] == WG_CELLS
        C = []
        C.append(("wg_1", _abi.batch3d_from_rois([_noise(rng, *g, levels=3) for g in WG_BOXES[:3]]), *_settings("radiomics")))
        C.append(("wg_2_3", _abi.batch3d_from_rois([_noise(rng, *g, levels=2) for g in WG_BOXES[3:6]]), *_settings("matlab")))
        C.append(("wg_4", _abi.batch3d_from_rois([_noise(rng, *WG_BOXES[6], levels=3, fill=0.8)]), *_settings("ibsi")))
        lanes = [_needle([n, 3], ax) for n in (LANES - 1, LANES, LANES + 1) for ax in (0, 1, 2)] + [_rows(n) for n in (LANES - 1, LANES, LANES + 1)]
        C.append(("lanes", _abi.batch3d_from_rois(lanes), *_settings("none", soft_nan=-3.25)))
        seg = [SHORT_RUNS - 1, SHORT_RUNS, SHORT_RUNS + 1, DENSE_SIZES - 1, DENSE_SIZES, DENSE_SIZES + 1, 2, 1, DENSE_SIZES + 1]
        C.append(("tables", _abi.batch3d_from_rois([_needle(seg, ax) for ax in (0, 1, 2)] + [_rows(3, w) for w in (DENSE_SIZES - 1, DENSE_SIZES, DENSE_SIZES + 1)]),
                  *_settings("mixed")))
        _CACHE["c"] = C
    return _CACHE["c"]
