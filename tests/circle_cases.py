"""Named inputs of the circle / geodetic tests (DIAMETER_MIN_ENCLOSING_CIRCLE, DIAMETER_CIRCUMSCRIBING_CIRCLE,
DIAMETER_INSCRIBING_CIRCLE, GEODETIC_LENGTH, THICKNESS): the same ROIs for the fixture generator (tests/golden/circle), the CPU tests
and the GPU tests.  Everything is rebuilt from seeds / parameters; the fixtures store outputs only.  Every ROI dict carries ABSOLUTE
coordinates: the circle class reads where the ROI lies (truncated midpoints, float roundings beyond 2^24).

Contour lengths of the small inputs, as the reference's ContourFeature gives them (recorded as `n_contour` in the fixtures and
asserted by tests/test_circle_cpu.py): one pixel 0, two pixels 0, an anti-diagonal 0 (the circle class skips these: three zeros);
three pixels in an L 2 (the two-point branch); three in a row 3; a 2 x 2 block 3; a 1 x 40 needle 40; a 12-pixel diagonal 12."""
from __future__ import annotations

import os

import numpy as np

from nyxus_amd import _abi
from tests import erosion_cases, synth
from tests.caliper_cases import _at
from tests.radial_cases import _mask_roi, comb, disc

HERE = os.path.dirname(os.path.abspath(__file__))
CONTOUR_LDS = 2048                   # kMomContourLds of nyxus_amd/csrc/roi_kernel.h: contour points the readers keep in LDS at most
RANDOM_SEED = 61
# (0, 0); two placements of the caliper tests; one beyond 2^24, where (float) x rounds
PLACEMENTS = [(0, 0), (4093, 60001), (1_000_003, 17), (16_777_300, 5)]
# name -> contour points (the ballot word boundaries of a wave): rows x columns of a filled box and the pixels of a bump on its top row
WORD_BOXES = {63: (30, 3, 2), 64: (3, 31, 0), 65: (31, 3, 2), 128: (3, 63, 0), 129: (61, 5, 1)}


def ell3():
    m = np.zeros((2, 2), bool)
    m[0, 0] = m[1, 0] = m[1, 1] = True
    return m


def box_bump(h, w, bump):
    m = np.ones((h + (1 if bump else 0), w), bool)
    if bump:
        m[0, :] = False
        m[0, :bump] = True
    return m


def plate():
    """A plate with a hole: a merged multicontour with a jump between the sub-contours."""
    m = np.ones((17, 23), bool)
    m[5:11, 6:15] = False
    return m


def checkerboard():
    """A checkerboard bridged by a full row and a full column."""
    yy, xx = np.mgrid[:11, :13]
    m = (xx + yy) % 2 == 0
    m[5, :] = True
    m[:, 6] = True
    return m


def spiral(turns=3.2, step=2.6):
    """A thin arm winding outwards: the contour walks ever farther from where it began, which sends the enclosing-circle search down
    to its third level again and again."""
    t = np.linspace(0.0, turns * 2 * np.pi, 4000)
    r = step * t / (2 * np.pi) * 2.0
    x, y = np.rint(r * np.cos(t)).astype(int), np.rint(r * np.sin(t)).astype(int)
    x, y = x - x.min(), y - y.min()
    m = np.zeros((y.max() + 1, x.max() + 1), bool)
    m[y, x] = True
    return m


def ring130():
    return disc(65) & ~np.pad(disc(50), 15)


def small_masks():
    return [np.ones((1, 1), bool), np.ones((1, 2), bool), np.ones((1, 3), bool), ell3(), np.ones((2, 2), bool), np.eye(3, dtype=bool)[::-1]]


def small():
    return [_mask_roi(m, 900 + i) for i, m in enumerate(small_masks())]


def shapes():
    ms = [np.ones((1, 40), bool), np.ones((40, 1), bool), np.eye(12, dtype=bool), disc(6), disc(30), plate(), checkerboard(), spiral(), comb(5, 9)]
    rois = [_mask_roi(m, 910 + i) for i, m in enumerate(ms)]
    rois.append(_mask_roi(disc(5), 925, const=7))
    return rois + synth.random_rois(8, seed=RANDOM_SEED, rmax=20)


def words():
    return [_mask_roi(box_bump(*WORD_BOXES[k]), 930 + i) for i, k in enumerate(sorted(WORD_BOXES))]


def long_comb():
    """Teeth two pixels wide: every tooth pixel is a contour point, more of them than the readers keep in LDS."""
    return [_mask_roi(comb(40, 30, spine=2), 940)]


def ring():
    return [_mask_roi(ring130(), 941)]


def mixed():
    """The ring (a box beyond the LDS contour plane: the big-box list chain) and the long comb beside small ROIs (the bulk chain)."""
    r = synth.random_rois(8, seed=RANDOM_SEED + 1, rmax=20)
    return r[:3] + ring() + r[3:6] + long_comb() + r[6:]


def placed_base():
    ms = small_masks()[2:5] + [np.ones((1, 40), bool), np.eye(12, dtype=bool), disc(6), plate(), checkerboard(), box_bump(*WORD_BOXES[65])]
    return [_mask_roi(m, 950 + i) for i, m in enumerate(ms)]


def placed():
    """The same shapes at four origins (placement-major)."""
    return [_at(r, ox, oy) for ox, oy in PLACEMENTS for r in placed_base()]


N_PLACED = 9


def tile():
    return erosion_cases.tile()


def tile_rois():
    it, lab = tile()
    return synth.rois_from_tile(it, lab)


CASES = {
    "small": small,
    "shapes": shapes,
    "words": words,
    "long_comb": long_comb,
    "ring": ring,
    "mixed": mixed,
    "placed": placed,
    "tile": tile_rois,
}
MIXED_RING, MIXED_COMB = 3, 7        # where the two large ROIs sit in "mixed"


def batch(name) -> _abi.HostBatch:
    return _abi.batch_from_rois(CASES[name]())


def golden():
    """{case: {"table": (n, 8) -- the five columns, PERIMETER, CENTROID_X, CENTROID_Y -- as recorded from the reference classes,
    "n_contour": (n,), "clamped": (n,) bool}}."""
    out = {}
    with np.load(os.path.join(HERE, "golden", "circle", "circle_reference.npz")) as z:
        for c in CASES:
            out[c] = {k: z[f"{c}__{k}"] for k in ("table", "n_contour", "clamped")}
        out["shapes_softnan"] = {"table": z["shapes_softnan__table"]}
    return out
