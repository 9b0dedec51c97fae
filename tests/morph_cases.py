"""Named inputs of the 2-D morphology tests (basic morphology, contour, convex hull, extrema: nyxhip_morph_batch / _tiles): the same
ROIs for the fixture generator (tests/golden/morph), the CPU tests and the GPU tests.  Everything is rebuilt from seeds / parameters;
the fixtures store outputs only.  Every ROI dict carries ABSOLUTE coordinates.  The shapes are those of tests/circle_cases.py and
tests/erosion_cases.py where they exist: the smallest inputs at which each path of roi_morph.hip can go wrong.

On import the module asserts that every sum x I and sum y I of every case, and the absolute shoelace terms of every hull, stay below
2^53: the reference's own sequential fp64 sums are then exact, and the exact-bits claims of the tests are claims about the kernel."""
from __future__ import annotations

import os

import numpy as np

from nyxus_amd import _abi
from tests import circle_cases, synth
from tests.caliper_cases import _at
from tests.radial_cases import _mask_roi, comb, disc

HERE = os.path.dirname(os.path.abspath(__file__))
CONTOUR_LDS = circle_cases.CONTOUR_LDS   # kMomContourLds: the contour readers' LDS bound
COLS_LDS = 1024                          # kMorphColsLds of nyxus_amd/csrc/roi_morph.h: box columns of the hull's tables in LDS
PLANE_LDS = 8192                         # kMorphPlaneLds: box cells of the intensity plane in LDS
RANDOM_SEED = 71
PLACEMENTS = [(0, 0), (4093, 60001), (1_000_003, 17), (1_048_576, 5)]
WORD_WIDTHS = [63, 64, 65, 128, 129, 1023, 1024, 1025]


def small_masks():
    """1 px, 2 px in a row, 3 in a row, an L of 3, 2 x 2, a 2-px anti-diagonal: no contour, n <= 2 standard deviations, the empty
    hull, +inf circularity."""
    return [np.ones((1, 1), bool), np.ones((1, 2), bool), np.ones((1, 3), bool), circle_cases.ell3(), np.ones((2, 2), bool),
            np.eye(2, dtype=bool)[::-1]]


def small():
    return [_mask_roi(m, 1100 + i) for i, m in enumerate(small_masks())]


def collinear():
    """Needles: two-vertex hulls whose area is the number of lattice points."""
    return [_mask_roi(m, 1110 + i) for i, m in enumerate([np.ones((1, 40), bool), np.ones((40, 1), bool), np.eye(12, dtype=bool)])]


def ring_mask():
    return disc(9) & ~np.pad(disc(5), 4)


def shapes():
    ms = [disc(3), disc(12), ring_mask(), comb(5, 9), circle_cases.plate(), circle_cases.spiral(), circle_cases.checkerboard()]
    rois = [_mask_roi(m, 1120 + i) for i, m in enumerate(ms)]
    rois.append(_mask_roi(disc(5), 1130, const=7))                           # flat intensities
    rois.append(_mask_roi(disc(4), 1131, const=0))                           # sum I = 0
    big = _mask_roi(np.ones((8, 8), bool), 1132)                             # 64 px, intensities up to 2^32 - 1
    v = np.random.default_rng(1132).integers(2 ** 31, 2 ** 32 - 1, 64, dtype=np.uint64).astype(np.uint32)
    v[5], v[40] = 2 ** 32 - 1, 2 ** 32 - 2
    rois.append(dict(big, inten=v))
    return rois


def octagon():
    m = np.ones((9, 11), bool)
    for k in range(3):
        m[k, :3 - k] = m[k, 8 + k:] = m[8 - k, :3 - k] = m[8 - k, 8 + k:] = False
    return m


def diamond(r=4):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return abs(xx) + abs(yy) <= r


def ties():
    """Top row, bottom row, left column and right column each hold several pixels | a single pixel each | an asymmetric one."""
    skew = np.zeros((7, 9), bool)
    skew[0, 2:5] = skew[6, 4:8] = True
    skew[1:6, 1:8] = True
    skew[2:4, 0] = skew[3:6, 8] = True
    return [_mask_roi(m, 1140 + i) for i, m in enumerate([octagon(), diamond(), skew])]


def words():
    return [_mask_roi(circle_cases.box_bump(2, w, 1), 1150 + i) for i, w in enumerate(WORD_WIDTHS)]


def long_comb():
    return circle_cases.long_comb()


def ring():
    return circle_cases.ring()


def mixed():
    return circle_cases.mixed()


def placed_base():
    return circle_cases.placed_base()


def placed():
    """The same nine shapes at four origins (placement-major)."""
    return [_at(r, ox, oy) for ox, oy in PLACEMENTS for r in placed_base()]


N_PLACED = circle_cases.N_PLACED


def tile():
    return circle_cases.tile()


def tile_rois():
    it, lab = tile()
    return synth.rois_from_tile(it, lab)


CASES = {
    "small": small,
    "collinear": collinear,
    "shapes": shapes,
    "ties": ties,
    "words": words,
    "long_comb": long_comb,
    "ring": ring,
    "mixed": mixed,
    "placed": placed,
    "tile": tile_rois,
}
MIXED_RING, MIXED_COMB = circle_cases.MIXED_RING, circle_cases.MIXED_COMB

_BATCHES = {}


def batch(name) -> _abi.HostBatch:
    """The case as a host batch (built once, shared, never modified)."""
    if name not in _BATCHES:
        _BATCHES[name] = _abi.batch_from_rois(CASES[name]())
    return _BATCHES[name]


def golden():
    """{case: {"table": (n, 41) as recorded from the reference classes (raw: +inf stays), "n_contour": (n,)}}."""
    out = {}
    with np.load(os.path.join(HERE, "golden", "morph", "morph_reference.npz")) as z:
        for c in CASES:
            out[c] = {k: z[f"{c}__{k}"] for k in ("table", "n_contour")}
    return out


def _check_exact_range():
    lim = 1 << 53
    for name in CASES:
        b = batch(name)
        for r in range(b.n_roi):
            o, e = int(b.px_offset[r]), int(b.px_offset[r + 1])
            ox = int(b.origin_x[r]) if b.origin_x is not None else 0
            oy = int(b.origin_y[r]) if b.origin_y is not None else 0
            v = b.inten[o:e].astype(object)
            sxi = int(((b.x[o:e].astype(object) + ox) * v).sum()) if e > o else 0
            syi = int(((b.y[o:e].astype(object) + oy) * v).sum()) if e > o else 0
            assert sxi < lim and syi < lim, (name, r, sxi, syi)
            # every shoelace term |x1 y2 - y1 x2| and their running sum: bounded by the hull's vertex count times the largest product
            xm, ym = ox + int(b.bbox_w[r]), oy + int(b.bbox_h[r])
            assert 2 * (int(b.bbox_w[r]) + int(b.bbox_h[r])) * xm * ym < lim, (name, r)


_check_exact_range()
