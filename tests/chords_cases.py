"""Named inputs of the chords tests (MAXCHORDS_*, ALLCHORDS_*): the same ROIs for the fixture generator (tests/golden/chords), the
CPU tests and the GPU tests.  Everything is rebuilt from seeds / parameters; the fixtures store outputs only.  Every ROI dict
carries ABSOLUTE coordinates: the chords depend on where the ROI lies (the reference rounds every rotated pixel coordinate to float
and truncates it toward zero)."""
from __future__ import annotations

import math
import os

import numpy as np

from nyxus_amd import _abi
from tests import synth
from tests.caliper_cases import PLACEMENTS, _at, degenerate, named_shapes, triangle  # noqa: F401  (the same small shapes)
from tests.radial_cases import _mask_roi, disc, tile_rois

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_WORDS = 8192                     # kChordsLdsWords of nyxus_amd/csrc/roi_chords.h: words of the rotated bit plane the kernel keeps in LDS
RANDOM_SEED = 41                     # (the generator replaces this seed, and nothing else, when a fixture is refused)


def plane_side(w, h):
    """chords_plane_side of roi_chords.h: no rotated box of a w x h box has a longer side."""
    q = int(w) * int(w) + int(h) * int(h)
    r = math.isqrt(q)
    return r + (r * r < q) + 2


def plane_words(w, h):
    """chords_plane_words of roi_chords.h: 32-bit words of the column-major bit plane of any rotation of a w x h box."""
    s = plane_side(w, h)
    return s * ((s + 31) // 32)


def shapes():
    return [_mask_roi(m, 300 + i) for i, m in enumerate(named_shapes())] + synth.random_rois(24, seed=RANDOM_SEED, rmax=25)


def placed():
    """The eight named shapes at three origins each (placement-major): (0, 0) gives negative rotated coordinates, the last one
    floats 0.0625 apart."""
    base = [_mask_roi(m, 300 + i) for i, m in enumerate(named_shapes())]
    return [_at(r, ox, oy) for ox, oy in PLACEMENTS for r in base]


COLLISION_ZEROS = (1, 9, 29)         # pixels (cloud order) of the 6 x 6 block that share a rotated cell with a non-zero pixel at some angle


def collision(reverse=False):
    """A 6 x 6 block: at 9 degrees pixels 0 and 1 land on one cell, and so do 3 and 9; at 162 degrees 29 and 35.  The second of
    each pair is zero: in cloud order the cell is a hole, in reversed order it is signal."""
    r = _mask_roi(np.ones((6, 6), bool), 77)
    r["inten"][list(COLLISION_ZEROS)] = 0
    if reverse:
        r = dict(x=r["x"][::-1].copy(), y=r["y"][::-1].copy(), inten=r["inten"][::-1].copy())
    return r


def zeros():
    stripe = _mask_roi(disc(16), 501)
    stripe["inten"][(stripe["x"] >= 14) & (stripe["x"] <= 16)] = 0           # a zero-intensity stripe: holes for the chords
    dark = _mask_roi(disc(5), 502, const=0)                                  # nothing but zeros: no chord at all
    rois = [stripe, dark, collision(), collision(reverse=True)]
    return [_at(r, 40 * i, 13 * i) for i, r in enumerate(rois)]


def _band(n):
    band = np.ones((3, n), bool)
    band[0, ::3] = False
    band[2, 1::4] = False
    return band


def step():
    """Rotated widths on both sides of 200 columns (step 1 -> 2), and a disc whose every rotation is wider."""
    ms = [_band(199), _band(200), _band(201), disc(110)]
    return [_at(_mask_roi(m, 600 + i), 5 * i, 3 * i) for i, m in enumerate(ms)]


def _thin(n):
    line = np.ones((1, n), bool)
    diag = np.zeros(((n - 4) // 8 + 1, n - 4), bool)                         # a thin diagonal: one step down every 8 columns
    diag[np.arange(n - 4) // 8, np.arange(n - 4)] = True
    return [line, _band(n), diag]


LIMIT_BELOW, LIMIT_ABOVE = (508, 509), (510, 547)


def limit():
    """Thin shapes whose planes just fit the LDS bit plane (the first half), and just do not (the second half: global planes)."""
    ms = [m for n in LIMIT_BELOW + LIMIT_ABOVE for m in _thin(n)]
    return [_at(_mask_roi(m, 700 + i), 11 * i, 7 * i) for i, m in enumerate(ms)]


CASES = {
    "degenerate": degenerate,
    "shapes": shapes,
    "zeros": zeros,
    "placed": placed,
    "step": step,
    "limit": limit,
    "tile": tile_rois,
}
N_NAMED = {"degenerate": 7, "shapes": 8, "zeros": 4, "placed": 24, "step": 4, "limit": 12, "tile": 0}   # ROIs that are not seeded


def batch(name) -> _abi.HostBatch:
    return _abi.batch_from_rois(CASES[name]())


def golden():
    """{case: {"table": (n, 16), "max": (n, 20) per-angle maxima (0: the angle gave no chord), "count" / "sum": (n, 20) number and sum
    of the angle's chords}} as recorded from the reference class."""
    out = {}
    with np.load(os.path.join(HERE, "golden", "chords", "chords_reference.npz")) as z:
        for c in CASES:
            out[c] = {k: z[f"{c}__{k}"] for k in ("table", "max", "count", "sum")}
        out["degenerate_softnan"] = {"table": z["degenerate_softnan__table"]}
    return out
