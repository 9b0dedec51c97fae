"""Edge cases of the volume texture kernels (roi_voltex.hip), rebuilt from seeds and held to tests/voltex_ref.py (no recording).  For
every constant at which a kernel changes form, an ROI one under, at and one over it:

  the cell range of one workgroup   kVtCellsPerWg = 32768 cells of the ROI's own box: boxes of 32767, 32768 and 32769 cells (one
                                    workgroup | one | two), 65535, 65536 and 65538 cells (two | two | three; 65537 is prime and a side
                                    ends at 65534) and 98306 cells (four).  The neighbours of a cell at the end of a range belong to
                                    the next workgroup's range; each workgroup merges its part into the ROI's table.
  the neighbourhood-class count     (radius + 1)^3 classes; a box side s against the radius r decides how many an axis has: s = r
                                    (every cube is clipped at both ends), r + 1, 2 r (one under the first cell with a whole cube),
                                    2 r + 1 (exactly one such cell) and 2 r + 2, for r = 1, 2, 3, mixed over the axes.

The sweeps stage nothing in LDS but their tables and index cells, not rows: there is no LDS-staging seam and no lanes-per-row switch in
this unit.

Each case is (name, batch, settings, texture settings)."""
from __future__ import annotations

import numpy as np

from nyxus_amd import _abi

CELLS_PER_WG = 32768         # kVtCellsPerWg of roi_voltex.h


def _roi(rng, w, h, d, fill=0.85, hi=60):
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    keep = rng.random(x.shape) < fill
    keep.flat[0] = keep.flat[-1] = True
    v = (1 + (x + 2 * y + 3 * z) % 7 * (hi // 8) + rng.integers(0, max(2, hi // 8), x.shape)).astype(np.uint32)
    v[rng.random(x.shape) < 0.02] = 0                      # zero-intensity voxels inside the cloud
    v.flat[0], v.flat[-1] = 1, hi
    return {"x": x[keep], "y": y[keep], "z": z[keep], "inten": v[keep], "origin": (0, 0, 0), "box": (w, h, d)}


def _settings(kind, radius, soft_nan=0.0):
    s = _abi.default_settings(32)
    s.soft_nan = soft_nan
    if kind == "radiomics":
        return s, _abi.VolTexSettings(-32, -32, radius)
    if kind == "matlab":
        return s, _abi.VolTexSettings(16, 16, radius)
    if kind == "mixed":                                    # two binned boxes
        return s, _abi.VolTexSettings(-24, 12, radius)
    s.ibsi = 1
    return s, _abi.VolTexSettings(0, 0, radius)


_CACHE = {}


def cases():
    if "c" not in _CACHE:
        rng = np.random.default_rng(20250219)
        C = []
        wg = [(7, 31, 151), (32, 32, 32), (331, 11, 9), (257, 17, 15), (64, 32, 32), (331, 66, 3), (199, 26, 19)]
        assert [w * h * d for w, h, d in wg] == [32767, 32768, 32769, 65535, 65536, 65538, 98306]
        C.append(("wg_1", _abi.batch3d_from_rois([_roi(rng, *g) for g in wg[:3]]), *_settings("radiomics", 1)))
        C.append(("wg_2_3", _abi.batch3d_from_rois([_roi(rng, *g) for g in wg[3:6]]), *_settings("matlab", 1)))
        C.append(("wg_4", _abi.batch3d_from_rois([_roi(rng, *wg[6])]), *_settings("ibsi", 1)))
        for r in (1, 2, 3):
            sides = [r, r + 1, 2 * r, 2 * r + 1, 2 * r + 2]
            boxes = [(sides[i], sides[(i + 1) % 5], sides[(i + 2) % 5]) for i in range(5)] + [(2 * r + 2, 2 * r + 3, 9), (1, 1, 2 * r + 2)]
            C.append((f"classes_r{r}", _abi.batch3d_from_rois([_roi(rng, *g) for g in boxes]), *_settings(("radiomics", "mixed", "ibsi")[r - 1], r, soft_nan=-3.25)))
        _CACHE["c"] = C
    return _CACHE["c"]
