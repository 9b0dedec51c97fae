"""Inputs of the whole-slide group tests (nyxhip_wsgroup_slides): the slides are rebuilt from seeds; the reference's tables for them
are tests/golden/wsgroup/wsgroup_reference.npz (make_wsgroup_golden.py)."""
import os

import numpy as np

from nyxus_amd import _abi
from tests.wholeslide_cases import _rng, slide

HERE = os.path.dirname(os.path.abspath(__file__))
B = _abi.WS_BAND_PIXELS
BW = 128                                        # the width of the band-seam cases: B / BW whole rows per band
assert B % BW == 0
BR = B // BW

# name -> (w, h, dtype, kind).  kinds: those of wholeslide_cases.slide, and big32 (uint32 with values above 2^31)
CASES = {
    # corners and the centre tie (even sides)
    "c1x1": (1, 1, np.uint8, "random"), "c1x9": (1, 9, np.uint16, "random"), "c9x1": (9, 1, np.uint8, "zeros"),
    "c2x2": (2, 2, np.uint32, "random"), "c3x3": (3, 3, np.uint8, "random"), "c4x4": (4, 4, np.uint16, "random"),
    "c5x8": (5, 8, np.uint32, "zeros"), "c16x16": (16, 16, np.uint8, "flat"), "c16x16z": (16, 16, np.uint16, "allzero"),
    # mid sizes: several tiles per band, odd sides, an odd pixel count in uint8
    "m257x33": (257, 33, np.uint16, "random"), "m33x257": (33, 257, np.uint32, "big32"), "m181x182": (181, 182, np.uint16, "zeros"),
    "m259x127": (259, 127, np.uint8, "random"),
    # the band cut: one band exactly, one row less / more, three bands with a short last one
    "b_exact": (BW, BR, np.uint8, "random"), "b_minus": (BW, BR - 1, np.uint16, "random"), "b_plus": (BW, BR + 1, np.uint32, "random"),
    "b_three": (BW, 2 * BR + 5, np.uint8, "zeros"),
}
NAN_CASES = {"c16x16z"}                         # an all-zero slide: the intensity variant divides by a zero mass


def image(name: str) -> np.ndarray:
    w, h, dt, kind = CASES[name]
    if kind == "big32":
        r = _rng(w, h, "big32")
        a = r.integers(0, 1 << 32, (h, w), dtype=np.uint64)
        a.flat[0] = (1 << 32) - 1
        a.flat[1] = (1 << 31) + 5
        return np.ascontiguousarray(a.astype(np.uint32))
    return slide(w, h, dt, kind)


def golden():
    z = np.load(os.path.join(HERE, "golden", "wsgroup", "wsgroup_reference.npz"))
    return {k: z[k] for k in z.files}
