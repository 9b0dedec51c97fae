"""Named inputs of the ellipse / erosion tests (MAJOR_AXIS_LENGTH .. ROUNDNESS, EROSIONS_2_VANISH[_COMPLEMENT]): the same ROIs for
the fixture generator (tests/golden/erosion), the CPU tests and the GPU tests.  Everything is rebuilt from seeds / parameters; the
fixtures store outputs only."""
from __future__ import annotations

import os

import numpy as np

from nyxus_amd import _abi
from tests import synth
from tests.radial_cases import _mask_roi, comb, disc

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_WORDS = 8192                     # kErosionLdsWords of nyxus_amd/csrc/roi_erosion.h: words of the TWO bit planes the kernel keeps in LDS
WAVE_PX = 2048                       # kEllipseWavePx: more pixels than this and a workgroup sums the ROI, not a wave
RANDOM_SEED = 52                     # (the generator replaces this seed, and nothing else, when a fixture is refused)
WIDTHS = (31, 32, 33, 64, 65)        # on both sides of the word boundaries of a row of w / 32 + 1 words


def plane_words(w, h):
    """erosion_plane_words of roi_erosion.h: words of ONE bit plane."""
    return (int(w) // 32 + 1) * int(h)


def ring():
    return disc(14) & ~np.pad(disc(6), 8)


def plus():
    m = np.zeros((15, 15), bool)
    m[5:10, :] = True
    m[:, 5:10] = True
    return m


def bar(w):
    """A frame row, column 1 and the last column full, and a bar three cells wide across the boundary between the row's first two
    words: after pass 0 only the bar's middle column is left of the updated cells, and only if the carries between words are right;
    what survives for ever sits in rows 0 and 1, column 1 and the last column."""
    m = np.zeros((12, w), bool)
    m[0, :] = True
    m[:, 1] = True
    m[:, w - 1] = True
    c = min(32, w - 3)
    m[:, c - 1:c + 2] = True
    return m


def cut(r, k):
    """A disc with a corner cut off: the box stays, the symmetry goes."""
    m = disc(r).copy()
    m[:k, :k] = False
    return m


def boxes():
    """Empty loops (3 x 3, 3 x 9, 9 x 3: value 0) and fixed points (4 x 4, 5 x 5, 40 x 7: value 1000).  (h, w) of numpy = (rows, columns)."""
    ms = [np.ones((3, 3), bool), np.ones((9, 3), bool), np.ones((3, 9), bool), np.ones((4, 4), bool), np.ones((5, 5), bool), np.ones((7, 40), bool)]
    return [_mask_roi(m, 800 + i) for i, m in enumerate(ms)]


def shapes():
    rois = [_mask_roi(m, 820 + i) for i, m in enumerate([disc(3), disc(12), ring(), plus(), comb(5, 9)])]
    z = _mask_roi(disc(6), 830)
    z["inten"][::3] = 0                                                      # zero-intensity pixels are mask all the same
    rois.append(z)
    rois.append(_mask_roi(disc(6), 831, const=7))                            # constant: the erosion class is skipped
    rois += [_mask_roi(bar(w), 840 + i) for i, w in enumerate(WIDTHS)]
    return rois


def dense(w, h, seed):
    m = np.random.default_rng(seed).random((h, w)) > 0.04
    m[0, :] |= True
    m[:, 0] |= True
    m[h - 1, w - 1] = True
    return m


def words():
    """Dense random masks on the word boundaries: a few holes, so the erosion runs some passes over every word."""
    return [_mask_roi(dense(w, 14 + 3 * i, RANDOM_SEED + i), 860 + i) for i, w in enumerate(WIDTHS)]


def thin_masks():
    needle = np.zeros((9, 33), bool)
    needle[np.arange(33) // 4, np.arange(33)] = True                         # one step down every 4 columns
    ell = np.zeros((9, 6), bool)
    ell[:, :2] = True
    ell[7:, :] = True
    return [np.ones((1, 1), bool), np.ones((1, 11), bool), np.ones((11, 1), bool), needle, ell]


def thin():
    return [_mask_roi(m, 880 + i) for i, m in enumerate(thin_masks())]


def sizes():
    """On both sides of the ellipse kernels' switch (2048 pixels), asymmetric."""
    return [_mask_roi(cut(25, 9), 890), _mask_roi(cut(26, 12), 891), _mask_roi(cut(27, 9), 892)]


def large():
    """One ROI whose two planes exceed the LDS bound (381 rows of 12 words, twice), and more pixels than a wave sums."""
    return [_mask_roi(cut(190, 120), 895)]


def mixed():
    """The large ROI beside small ones: the list launch and the LDS launch in one call."""
    r = synth.random_rois(10, seed=RANDOM_SEED, rmax=20)
    return r[:5] + large() + r[5:]


def tile():
    """A 256 x 256 label tile of asymmetric shapes on a 64-pixel grid (the discs of radial_cases.tile() are exactly symmetric: their
    ORIENTATION and ECCENTRICITY are the values the fixtures do not compare) and its intensities."""
    ms = [cut(25, 9), cut(14, 6), thin_masks()[3], thin_masks()[4], bar(33), dense(31, 20, RANDOM_SEED + 9), dense(33, 17, RANDOM_SEED + 10)]
    for r in synth.random_rois(9, seed=RANDOM_SEED + 1, rmax=20):
        m = np.zeros((int(r["y"].max()) + 1, int(r["x"].max()) + 1), bool)
        m[r["y"], r["x"]] = True
        ms.append(m)
    lab = np.zeros((256, 256), np.uint32)
    for i, m in enumerate(ms):
        oy, ox = 64 * (i // 4) + 3 + i % 5, 64 * (i % 4) + 2 + i % 7
        lab[oy:oy + m.shape[0], ox:ox + m.shape[1]][m] = i + 1
    return synth.intensity_tile(5, size=256), lab


def tile_rois():
    it, lab = tile()
    return synth.rois_from_tile(it, lab)


CASES = {
    "boxes": boxes,
    "shapes": shapes,
    "words": words,
    "thin": thin,
    "sizes": sizes,
    "large": large,
    "mixed": mixed,
    "tile": tile_rois,
}
# ROIs that are asymmetric on purpose (no masked value allowed), and the seeded ones (at most 10 % with a masked value)
ASYMMETRIC = {"boxes": [], "shapes": [], "words": [], "thin": [3, 4], "sizes": [0, 1, 2], "large": [0], "mixed": [5], "tile": []}
RANDOM = {"boxes": [], "shapes": [], "words": [0, 1, 2, 3, 4], "thin": [], "sizes": [], "large": [], "mixed": [0, 1, 2, 3, 4, 6, 7, 8, 9, 10], "tile": None}


def random_indices(name, n):
    return list(range(n)) if RANDOM[name] is None else RANDOM[name]


def batch(name) -> _abi.HostBatch:
    return _abi.batch_from_rois(CASES[name]())


def golden():
    """{case: {"table": (n, 8) as recorded from the reference classes, "compared": (n, 8) bool}}."""
    out = {}
    with np.load(os.path.join(HERE, "golden", "erosion", "erosion_reference.npz")) as z:
        for c in CASES:
            out[c] = {k: z[f"{c}__{k}"] for k in ("table", "compared")}
        out["shapes_softnan"] = {"table": z["shapes_softnan__table"]}
    return out
