"""Named inputs of the radial-distribution tests: the same ROIs for the fixture generator (tests/golden/radial), the CPU
tests and the GPU tests.  Everything is rebuilt from seeds / parameters; the fixtures store outputs only."""
from __future__ import annotations

import json
import os

import numpy as np

from nyxus_amd import _abi
from tests import fixtures, synth

HERE = os.path.dirname(os.path.abspath(__file__))


def _cm(x, y, v):
    """ROI dict in column-major pixel order (the in-memory workflow's scan order, phase2_2d.cpp:655-656)."""
    x, y, v = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(v, np.uint32)
    o = np.lexsort((y, x))
    return dict(x=x[o], y=y[o], inten=v[o])


def _mask_roi(m, seed, hi=4096, const=None):
    y, x = np.nonzero(m)
    v = np.full(len(x), const, np.uint32) if const is not None else np.random.default_rng(seed).integers(1, hi, len(x)).astype(np.uint32)
    return _cm(x, y, v)


def disc(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return xx * xx + yy * yy <= r * r


def comb(teeth, length, spine=6):
    m = np.zeros((length + spine, 4 * teeth), bool)
    m[:spine] = True
    for t in range(teeth):
        m[spine:, 4 * t:4 * t + 2] = True
    return m


def shape2d():
    ref = json.load(open(os.path.join(HERE, "golden", "reference_tests.json")))
    return [fixtures.roi_from_triplets(ref["pixels"]["shape2d_morphology_intensity"], ref["pixels"]["shape2d_morphology_mask"])]


def special():
    """Holes, a constant ROI, a single pixel, lines, shapes without a closed contour."""
    ring = disc(14) & ~np.pad(disc(6), 8)
    sieve = disc(12).copy()
    sieve[::3, ::3] = False
    line = np.ones((1, 17), bool)
    diag = np.eye(6, dtype=bool)
    ell = np.zeros((7, 7), bool)
    ell[:, 0] = True
    ell[6, :] = True
    return [_mask_roi(ring, 1), _mask_roi(sieve, 2), _mask_roi(disc(9), 3, const=7), _mask_roi(np.ones((1, 1), bool), 4),
            _mask_roi(line, 5), _mask_roi(line.T, 6), _mask_roi(diag, 7), _mask_roi(ell, 8), _mask_roi(np.ones((1, 2), bool), 9),
            _mask_roi(np.ones((2, 2), bool), 10), _mask_roi(np.ones((3, 3), bool), 11)]


def heavy():
    """A heavy-tailed batch: small random ROIs beside a disc beyond the LDS contour plane and pixel staging (r = 80: 20 k pixels,
    a 163 x 163 padded plane), one staged wide (r = 35: 3.8 k pixels), and a comb whose contour has several thousand points."""
    rois = synth.random_rois(12, seed=21, rmax=20)
    rois += [_mask_roi(disc(80), 31), _mask_roi(disc(35), 32), _mask_roi(comb(40, 110), 33), _mask_roi(comb(12, 40), 34, hi=2 ** 32 - 1)]
    return rois


def tile():
    """A 256 x 256 label tile (irregular discs, some concave) and its intensities; the ROIs as the workflow assembles them."""
    lab = synth.disk_label_tile(size=256, irregular=True, seed=2)
    it = synth.intensity_tile(5, size=256)
    return it, lab


def tile_rois():
    it, lab = tile()
    return synth.rois_from_tile(it, lab)


CASES = {
    "shape2d": shape2d,
    "rand_seed3_rmax12": lambda: synth.random_rois(40, seed=3, rmax=12),
    "rand_seed9_rmax25": lambda: synth.random_rois(40, seed=9, rmax=25),
    "rand_seed5_rmax40": lambda: synth.random_rois(40, seed=5, rmax=40),
    "special": special,
    "heavy": heavy,
    "tile": tile_rois,
}


def batch(name) -> _abi.HostBatch:
    return _abi.batch_from_rois(CASES[name]())


def golden():
    """{case: {"table": (n, 24), "dst2": (n,), "n_contour": (n,)}} as recorded from the reference classes."""
    with np.load(os.path.join(HERE, "golden", "radial", "radial_reference.npz")) as z:
        return {c: {k: z[f"{c}__{k}"] for k in ("table", "dst2", "n_contour")} for c in CASES}
