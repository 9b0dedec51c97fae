"""Named inputs of the hexagonality / polygonality tests (POLYGONALITY_AVE, HEXAGONALITY_AVE, HEXAGONALITY_STDDEV): the same label
images for the fixture generator (tests/golden/hexpoly), the CPU tests and the GPU tests.  Everything is rebuilt from parameters; the
fixtures store the six inputs and the three outputs of every ROI.

A case is a stack of equally sized label images (one image = one tile of the tile entry = one CSR range of the batch entry), the
neighbor radius it runs at, and optionally an origin its batch is moved to (batch entry only).  They are the smallest scenes in which
each branch of the class can go wrong:
  lattice        5 x 5 boxes of 5 x 5 pixels at gap 2, R = 5: 3 (corners), 5 (edges) and 8 (inside) neighbors
  low_counts     a row of four boxes (1 and 2 neighbors: -1) and an isolated box (0 neighbors: -1)
  no_contour     a single pixel and a two-pixel ROI (empty contours: -1) inside a crowd of boxes
  needle         a 1 x 9 needle with five neighbors: the degenerate Feret diameters
  beyond_table   a 1 x 400 bar between two rows of 1 x 3 ROIs at every second column: about 400 neighbors, beyond the tangent table
  hex_discs      hexagonally packed discs of radius 6: the middle one has 6 neighbors and a clean score
  deferred       a bar wider than the caliper kernel's LDS column table and a box beyond the morphology kernel's LDS plane, each
                 with three neighbors or more (the deferred lists of both kernels)
  three_images   three images in one batch: the ROIs of different images are never neighbors
  far            the lattice at an origin beyond 2^24"""
from __future__ import annotations

import json
import os

import numpy as np

from nyxus_amd import _abi
from tests.neighbors_cases import batch_of_images, intensity, put
from tests.radial_cases import disc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "hexpoly")
FAR_X = 16_777_300                   # beyond 2^24: the origin the "far" case is moved to
CALIPER_COLS_LDS = 1024              # kCaliperColsLds (roi_caliper.h), kMorphColsLds (roi_morph.h)
MORPH_PLANE_LDS = 8192               # kMorphPlaneLds
BOX = np.ones((5, 5), bool)


def lattice(n=5):
    lab = np.zeros((7 * n + 5, 7 * n + 5), np.uint32)
    for i in range(n):
        for j in range(n):
            put(lab, BOX, 3 + 7 * i, 3 + 7 * j, 1 + n * i + j)
    return [lab]


def low_counts():
    lab = np.zeros((40, 48), np.uint32)
    for k in range(4):
        put(lab, BOX, 4, 3 + 7 * k, k + 1)
    put(lab, BOX, 30, 38, 9)
    return [lab]


def no_contour():
    """Eight boxes around a hole that holds a single pixel and a two-pixel ROI: every box is within R = 5 of both."""
    lab = np.zeros((32, 32), np.uint32)
    k = 0
    for i in range(3):
        for j in range(3):
            if (i, j) != (1, 1):
                k += 1
                put(lab, BOX, 3 + 7 * i, 3 + 7 * j, k)
    put(lab, np.ones((1, 1), bool), 11, 11, 20)
    put(lab, np.ones((1, 2), bool), 13, 12, 21)
    return [lab]


def needle():
    lab = np.zeros((24, 32), np.uint32)
    put(lab, np.ones((1, 9), bool), 11, 11, 1)
    put(lab, BOX, 4, 8, 2); put(lab, BOX, 4, 15, 3); put(lab, BOX, 14, 8, 4); put(lab, BOX, 14, 15, 5)
    put(lab, BOX, 9, 22, 6)
    return [lab]


def beyond_table():
    lab = np.zeros((12, 408), np.uint32)
    put(lab, np.ones((1, 400), bool), 5, 4, 1)
    for k in range(200):
        put(lab, np.ones((3, 1), bool), 1, 4 + 2 * k, 2 + k)
        put(lab, np.ones((3, 1), bool), 7, 4 + 2 * k, 202 + k)
    return [lab]


def hex_discs():
    lab = np.zeros((48, 64), np.uint32)
    k = 0
    for row, (y, xs) in enumerate(((2, (9, 23, 37)), (14, (2, 16, 30, 44)), (26, (9, 23, 37)))):
        for x in xs:
            k += 1
            put(lab, disc(6), y, x, k)
    return [lab]


HEX_MIDDLE = (5, 6)                  # labels of the two discs of the middle row that have six neighbors


def deferred():
    lab = np.zeros((128, 1120), np.uint32)
    put(lab, np.ones((2, 1100), bool), 4, 8, 1)                               # wider than both column tables
    put(lab, BOX, 8, 20, 2); put(lab, BOX, 8, 500, 3); put(lab, BOX, 8, 1000, 4)
    put(lab, np.ones((100, 100), bool), 20, 8, 5)                             # 10000 cells: beyond the morphology kernel's LDS plane
    put(lab, BOX, 30, 110, 6); put(lab, BOX, 60, 110, 7); put(lab, BOX, 122, 40, 8); put(lab, BOX, 90, 110, 9)
    return [lab]


def three_images():
    a = lattice(3)[0]
    b = np.zeros_like(a)
    b[1:, :] = np.where(a[:-1, :] > 0, 7 * a[:-1, :].astype(np.int64) + 3, 0).astype(np.uint32)   # the same boxes a row lower, other labels
    c = np.zeros_like(a)
    put(c, disc(6), 2, 2, 100001); put(c, BOX, 3, 17, 100002); put(c, BOX, 10, 17, 100003); put(c, BOX, 17, 10, 100004); put(c, BOX, 17, 3, 100005)
    return [a, b, c]


# name -> (builder, radius, origin)
CASES = {
    "lattice": (lattice, 5, None),
    "low_counts": (low_counts, 5, None),
    "no_contour": (no_contour, 5, None),
    "needle": (needle, 5, None),
    "beyond_table": (beyond_table, 5, None),
    "hex_discs": (hex_discs, 5, None),
    "deferred": (deferred, 5, None),
    "three_images": (three_images, 5, None),
    "far": (lattice, 5, (FAR_X, 7)),
}
API_CASE = "three_images"            # the stack behind api_expected.json


def images(name):
    return CASES[name][0]()


def radius(name):
    return CASES[name][1]


def stack(name):
    """(I, M): the [n_images, H, W] stacks of the tile entry."""
    M = np.stack(images(name))
    I = np.stack([intensity(m, 500 + k) for k, m in enumerate(M)])
    return I, M


def batch(name) -> _abi.HostBatch:
    return batch_of_images(images(name), CASES[name][2])


def golden():
    """{case: (inputs (n_roi, 7) in the order of hexpoly_ref.INPUTS, outputs (n_roi, 3))} and the synthetic sweep under "sweep", as
    recorded from the reference's class."""
    with np.load(os.path.join(GOLDEN_DIR, "hexpoly_reference.npz")) as z:
        return {name: (z[f"{name}__in"], z[f"{name}__out"]) for name in list(CASES) + ["sweep"]}


def api_expected():
    return json.load(open(os.path.join(GOLDEN_DIR, "api_expected.json")))


def sweep(seed=20240, n=2000):
    """About n synthetic rows of hexpoly_ref.INPUTS: random shapes' numbers at every neighbor count that takes another path (0 .. 5, the
    table's last entry 128, the first beyond it 129, 1000), then the degenerate ones -- no contour, a Feret minimum of 0, a hull area
    of 0, a perimeter of 0, huge and tiny areas."""
    rng = np.random.default_rng(seed)
    counts = [0, 1, 2, 3, 4, 5, 6, 8, 128, 129, 1000]
    rows = []
    for i in range(n):
        nb = counts[i % len(counts)] if i % 3 else int(rng.integers(0, 200))
        r = float(rng.uniform(1.0, 60.0))
        px = max(1, int(np.pi * r * r * rng.uniform(0.5, 1.2)))
        per = float(2 * np.pi * r * rng.uniform(0.7, 2.5))
        hull = float(px * rng.uniform(1.0, 1.6)) + 1.0
        fmin = float(2 * r * rng.uniform(0.3, 1.0))
        fmax = float(fmin * rng.uniform(1.0, 3.0))
        nk = int(per) + 1
        kind = i % 40
        if kind == 7: nk = 0
        elif kind == 11: fmin = 0.0
        elif kind == 13: hull = 0.0
        elif kind == 17: per = 0.0
        elif kind == 19: px, hull = int(rng.integers(2 ** 31, 2 ** 32 - 1)), float(2.0 ** 40 * rng.uniform(1, 2))
        elif kind == 23: px, hull, per, fmin, fmax = 3, 1.0 + 1e-9, 1e-7, 1e-9, 1e-8
        elif kind == 29: fmin = fmax = 0.0
        elif kind == 31: per, fmax = 1e300, 1e300
        rows.append([px, nk, nb, per, hull, fmin, fmax])
    return np.asarray(rows, np.float64)
