"""Named inputs of the caliper tests (Feret, Martin and Nassenstein diameters): the same ROIs for the fixture generator
(tests/golden/caliper), the CPU tests and the GPU tests.  Everything is rebuilt from seeds / parameters; the fixtures store outputs
only.  Every ROI dict carries ABSOLUTE coordinates: the caliper values depend on where the ROI lies (the reference rounds every
rotated hull vertex to float)."""
from __future__ import annotations

import os

import numpy as np

from nyxus_amd import _abi
from tests import synth
from tests.outline_cases import ring, two_holes
from tests.radial_cases import _mask_roi, disc, tile_rois

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_COLS = 1024                      # kCaliperColsLds of nyxus_amd/csrc/roi_caliper.h: box columns whose tables the kernel keeps in LDS
PLACEMENTS = [(0, 0), (4093, 60001), (1_000_003, 17)]


def _m(rows):
    return np.array(rows, bool)


def triangle(n=9):
    return np.tril(np.ones((n, n), bool))


def _at(roi, ox, oy):
    return dict(roi, x=roi["x"] + ox, y=roi["y"] + oy)


def degenerate():
    """Hulls of 0, 2, 3 and 4 vertices."""
    shapes = [
        _m([[1]]),                                       # 1 pixel: no hull, soft_nan everywhere
        _m([[1, 1]]),                                    # 2 pixels
        np.ones((1, 5), bool), np.ones((5, 1), bool), np.eye(5, dtype=bool),   # lines: hulls of 2 vertices
        np.ones((2, 2), bool),
        _m([[1, 0], [1, 1]]),                            # a 3-pixel L
    ]
    return [_mask_roi(m, 200 + i) for i, m in enumerate(shapes)]


def named_shapes():
    plate = two_holes()
    return [np.ones((3, 7), bool), np.ones((7, 3), bool), triangle(), disc(3), disc(16), disc(33), ring(), plate]


RANDOM_SEED = 31                     # (the generator replaces this seed, and nothing else, when a fixture is refused)


def shapes():
    return [_mask_roi(m, 300 + i) for i, m in enumerate(named_shapes())] + synth.random_rois(24, seed=RANDOM_SEED, rmax=25)


def placed():
    """The eight named shapes at three origins each (placement-major)."""
    base = [_mask_roi(m, 300 + i) for i, m in enumerate(named_shapes())]
    return [_at(r, ox, oy) for ox, oy in PLACEMENTS for r in base]


def _wide(n):
    line = np.ones((1, n), bool)
    band = np.ones((3, n), bool)
    band[0, ::3] = False
    band[2, 1::4] = False
    band[0, 0] = band[2, 0] = band[0, -1] = band[2, -1] = True
    diag = np.zeros((n // 8 + 1, n), bool)               # a thin diagonal: one step down every 8 columns
    diag[np.arange(n) // 8, np.arange(n)] = True
    return [line, band, diag]


def wide():
    """Boxes just below and just above the LDS column table (the second half goes through the global tables)."""
    ms = _wide(LDS_COLS - 1) + _wide(LDS_COLS) + _wide(LDS_COLS + 1) + _wide(LDS_COLS + 37)
    return [_at(_mask_roi(m, 400 + i), 11 * i, 7 * i) for i, m in enumerate(ms)]


CASES = {
    "degenerate": degenerate,
    "shapes": shapes,
    "placed": placed,
    "wide": wide,
    "tile": tile_rois,
}


def batch(name) -> _abi.HostBatch:
    return _abi.batch_from_rois(CASES[name]())


def golden():
    """{case: {"table": (n, 20), "hull": [n arrays (k, 2) of relative vertices], "feret" / "martin" / "nassenstein": (n, 19) per-angle
    diameters (NaN: the angle gave none)}} as recorded from the reference classes."""
    out = {}
    with np.load(os.path.join(HERE, "golden", "caliper", "caliper_reference.npz")) as z:
        for c in CASES:
            off = z[f"{c}__hull_offset"]
            pts = z[f"{c}__hull_points"]
            out[c] = {"table": z[f"{c}__table"], "hull": [pts[off[i]:off[i + 1]] for i in range(len(off) - 1)],
                      "feret": z[f"{c}__feret"], "martin": z[f"{c}__martin"], "nassenstein": z[f"{c}__nassenstein"]}
        out["degenerate_softnan"] = {"table": z["degenerate_softnan__table"]}
    return out
