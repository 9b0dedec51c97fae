"""Edge cases of the volume distance-zone kernels (roi_voldzone.hip), rebuilt from seeds and held to tests/voldzone_ref.py (no recording).
For every constant at which a kernel changes form, an ROI on either side of it:

  the cell range of one workgroup   W = kVzCellsPerWg = 4096 cells of the ROI's own box: boxes of W - 1 and W cells (one workgroup), and
                                    of W + 1 and 2W + 2 cells (two | three).  Three levels of noise over a sparse cloud; and for each
                                    range seam and each raster-earlier face neighbour (-x, -y, -z) of the range's first cell that the
                                    box has, a copy of the box in which that pair alone carries level 99: a zone of two cells that
                                    crosses the seam through that neighbour (SEAMS lists them).
  the lanes of the closing          distance j + 1 belongs to lane j % 64: planes of 125 x 125, 127 x 127 and 129 x 129 cells of one
                                    level with a single voxel of another level at the centre, so that Nd is 63, 64 and 65.
  the LDS table of the emit step    metrics up to kVdzShortDist = 8 are counted in LDS: single-voxel zones of metric 7, 8 and 9 beside
                                    the centre of a 17 x 17 plane.
  degenerate ROIs                   flat ROIs and an ROI without voxels under a non-zero soft_nan.

Each case is (name, batch, settings)."""
from __future__ import annotations

import numpy as np

from nyxus_amd import _abi
from tests.voldzone_cases import LANES, SHORT_DIST, W, roi_from_cube, settings, with_empty

CELLS_PER_WG = W
WG_BOXES = [(21, 15, 13), (16, 16, 16), (241, 17, 1), (241, 17, 2)]   # (w, h, d)
WG_CELLS = [W - 1, W, W + 1, 2 * W + 2]
SEAM_LEVEL = 99


def earlier_face_neighbours(c, w, h, d):
    """{axis: flat index} of the face neighbours of cell c that come before it in raster order"""
    z, y, x = c // (w * h), c // w % h, c % w
    out = {}
    if x > 0:
        out["x"] = c - 1
    if y > 0:
        out["y"] = c - w
    if z > 0:
        out["z"] = c - w * h
    return out


def _noise(rng, w, h, d, pair=None, fill=0.9):
    V = rng.integers(1, 4, (d, h, w)) * 9
    keep = rng.random(V.shape) < fill
    keep.flat[0] = keep.flat[-1] = True
    V.flat[0], V.flat[-1] = 9, 27
    if pair is not None:
        for q in pair:
            V.flat[q] = SEAM_LEVEL
            keep.flat[q] = True
    return roi_from_cube(V, keep)


def _plane(side, marks):
    """a side x side x 1 plane of level 5 with single voxels (x, y, level)"""
    V = np.full((1, side, side), 5)
    for x, y, lv in marks:
        V[0, y, x] = lv
    return roi_from_cube(V)


_CACHE = {}


def seams():
    """(ROI index in the "wg" case, first cell of the range, its neighbour, axis) of every seam-crossing pair"""
    cases()
    return _CACHE["seams"]


def cases():
    if "c" not in _CACHE:
        rng = np.random.default_rng(20250404)
        assert [w * h * d for w, h, d in WG_BOXES] == WG_CELLS
        rois, S = [_noise(rng, *g) for g in WG_BOXES], []
        for g in WG_BOXES:
            cells = g[0] * g[1] * g[2]
            for c in range(W, cells, W):
                for ax, q in earlier_face_neighbours(c, *g).items():
                    S.append((len(rois), c, q, ax))
                    rois.append(_noise(rng, *g, pair=(c, q)))
        assert {ax for _, _, _, ax in S} == {"x", "y", "z"}
        _CACHE["seams"] = S
        C = [("wg", _abi.batch3d_from_rois(rois), settings("none"))]
        C.append(("lanes", _abi.batch3d_from_rois([_plane(2 * n - 1, [(n - 1, n - 1, 9)]) for n in (LANES - 1, LANES, LANES + 1)]), settings("ibsi")))
        n = SHORT_DIST + 1                                 # the centre of a 17 x 17 plane has metric 9, its left neighbours 8 and 7
        C.append(("emit", _abi.batch3d_from_rois([_plane(2 * n - 1, [(n - 1, n - 1, 9), (n - 2, n - 1, 10), (n - 3, n - 1, 11)])]), settings("matlab")))
        flat = [roi_from_cube(np.full((2, 3, 4), 6)), roi_from_cube(np.full((1, 1, 1), 1)), roi_from_cube(np.zeros((2, 2, 2), np.int64)),
                roi_from_cube(np.array([[[1, 2, 2], [2, 1, 1]]]))]
        C.append(("degenerate", with_empty(_abi.batch3d_from_rois(flat), at=1), settings("softnan")))
        _CACHE["c"] = C
    return _CACHE["c"]
