"""Named inputs of the outline tests (fractal dimensions, Euler number, ROI radius): the same ROIs for the fixture generator
(tests/golden/outline), the CPU tests and the GPU tests.  Everything is rebuilt from seeds / parameters; the fixtures store
outputs only."""
from __future__ import annotations

import os

import numpy as np

from nyxus_amd import _abi
from tests import synth
from tests.radial_cases import _mask_roi, comb, disc, tile_rois

HERE = os.path.dirname(os.path.abspath(__file__))


def _m(rows):
    return np.array(rows, bool)


def ring():
    """One hole: Euler number 0."""
    return disc(10) & ~np.pad(disc(4), 6)


def two_holes():
    """A plate with two holes: Euler number -1."""
    m = np.ones((9, 15), bool)
    m[3:6, 3:6] = False
    m[3:6, 9:12] = False
    return m


def checker():
    """A 4 x 4 checkerboard of 2 x 2 blocks, joined by one-pixel bridges: diagonal contacts, many small holes."""
    m = np.zeros((8, 8), bool)
    for r in range(4):
        for c in range(4):
            if (r + c) % 2 == 0:
                m[2 * r:2 * r + 2, 2 * c:2 * c + 2] = True
    m[1, 2] = m[3, 4] = m[5, 2] = m[6, 5] = True
    return m


def box_with_notches(side):
    """A filled square of `side` with a few cells missing at the border and one hole: the box counts of the coarse scales stay full,
    the fine ones do not."""
    m = np.ones((side, side), bool)
    m[0, 1::5] = False
    m[side // 2, side // 2] = False
    m[-1, ::7] = False
    m[-1, 0] = True                     # (the bounding box stays side x side)
    m[-1, -1] = True
    return m


def small():
    """The smallest shapes that can go wrong: counts of pixels, quads and contour points at their edges."""
    shapes = [
        _m([[1]]),                                      # 1 pixel: no contour
        _m([[1, 1]]),                                   # 2 pixels side by side
        _m([[1, 0], [0, 1]]),                           # 2 pixels on a diagonal: one object in mode 8
        np.ones((1, 17), bool), np.ones((17, 1), bool),   # 1 x N, N x 1
        np.ones((8, 8), bool),                          # a full box
        ring(), two_holes(), checker(),
        np.ones((3, 1), bool),                          # contours of 3, 4, 7, 8 points: zero, one, one and two strides of the divider walk
        np.ones((4, 1), bool),
        _m([[1, 0], [1, 1], [1, 1], [1, 1]]),
        np.ones((2, 4), bool),
    ]
    shapes += [box_with_notches(s) for s in (32, 33, 64, 65)]   # shifting grids | one grid, and a word boundary of the bit plane
    return [_mask_roi(m, 100 + i) for i, m in enumerate(shapes)]


def heavy():
    """The HBM paths: a disc beyond the staged pixels (r = 40: 5 k pixels), a comb whose contour exceeds the LDS contour, and a
    300 x 300 plate with holes, beyond the LDS contour plane and the LDS bit planes."""
    plate = np.ones((300, 300), bool)
    plate[20:40, 30:90] = False
    plate[100:220, 140:160] = False
    plate[250:260, 250:260] = False
    plate[0, ::3] = False
    plate[0, 0] = plate[0, -1] = True
    return synth.random_rois(6, seed=23, rmax=20) + [_mask_roi(disc(40), 41), _mask_roi(comb(40, 110), 42), _mask_roi(plate, 43)]


CASES = {
    "small": small,
    "rand_seed17_rmax25": lambda: synth.random_rois(30, seed=17, rmax=25),
    "heavy": heavy,
    "tile": tile_rois,
}

NAMES = ["FRACT_DIM_BOXCOUNT", "FRACT_DIM_PERIMETER", "EULER_NUMBER", "ROI_RADIUS_MEAN", "ROI_RADIUS_MAX", "ROI_RADIUS_MEDIAN"]
EXACT = ("EULER_NUMBER", "ROI_RADIUS_MAX", "ROI_RADIUS_MEDIAN")
DIM_ATOL = 1e-5          # the two dimensions: O(1) quotients of cancelling sums of logarithms (relative OR this absolute bound)


def batch(name) -> _abi.HostBatch:
    return _abi.batch_from_rois(CASES[name]())


def golden():
    """{case: {"table": (n, 6), "n_contour": (n,), "box_counts": (n, 5, 4)}} as recorded from the reference classes.  box_counts:
    the four shifted-grid counts per box size 32, 16, 8, 4, 2 of the ROIs whose padded side is <= 32 (-1 elsewhere)."""
    with np.load(os.path.join(HERE, "golden", "outline", "outline_reference.npz")) as z:
        return {c: {k: z[f"{c}__{k}"] for k in ("table", "n_contour", "box_counts")} for c in CASES}


def mismatches(got, want, rel):
    """Rows / columns of two (n, 6) tables that differ beyond the bounds of the outline tests: the integer columns exactly,
    ROI_RADIUS_MEAN within `rel`, the two dimensions within `rel` relative or DIM_ATOL absolute.  NaN in `want` = not compared
    (the reference is undefined there)."""
    bad = []
    for c, name in enumerate(NAMES):
        g, w = got[:, c], want[:, c]
        use = ~np.isnan(w)
        if name in EXACT:
            ok = g == w
        elif name == "ROI_RADIUS_MEAN":
            ok = np.abs(g - w) <= rel * np.abs(w)
        else:
            ok = (np.abs(g - w) <= rel * np.abs(w)) | (np.abs(g - w) <= DIM_ATOL)
        for r in np.nonzero(use & ~ok)[0]:
            bad.append(f"row {r} {name}: got {g[r]!r}, want {w[r]!r}")
    return bad
