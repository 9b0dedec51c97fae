"""Named inputs of the neighbor tests (NUM_NEIGHBORS .. ANG_BW_NEIGHBORS_MODE): the same label images for the fixture generator
(tests/golden/neighbors), the CPU tests and the GPU tests.  Everything is rebuilt from parameters; the fixtures store outputs only.

A case is a stack of equally sized label images (one image = one tile of the tile entry = one CSR range of the batch entry), the
radii it is recorded at, and optionally an origin its batch is moved to (batch entry only: a tile's ROIs lie where they lie).
Every image is at most 96 x 96 except the comb (48 x 176) and the ring (160 x 160), whose ROIs are the large ones of
tests/circle_cases.py."""
from __future__ import annotations

import json
import os

import numpy as np

from nyxus_amd import _abi
from tests import synth
from tests.circle_cases import WORD_BOXES, box_bump, checkerboard, ring130
from tests.radial_cases import comb, disc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "neighbors")
FAR_X = 16_777_300                   # beyond 2^24: the origin the "placed" case is moved to


def put(lab, m, y, x, label):
    """Paints mask m with its top left corner at (y, x); the target must be free."""
    m = np.asarray(m, bool)
    h, w = m.shape
    assert y >= 0 and x >= 0 and y + h <= lab.shape[0] and x + w <= lab.shape[1], (label, y, x, m.shape, lab.shape)
    win = lab[y:y + h, x:x + w]
    assert not (win[m] != 0).any(), label
    win[m] = label


BOX = np.ones((5, 5), bool)


def contacts():
    """Pairs of 5 x 5 boxes at chosen distances, each pair 16 pixels or more from the next (alone at every recorded radius), and one
    isolated box.  Labels: pair k holds 10 k + 1 and 10 k + 2.
      pair 1  edge contact (d = 1)            pair 2  diagonal-only contact (d = 2)     pair 3  a one-pixel gap (d = 4)
      pair 4  contour distance 5 (d = 25)     pair 5  contour distance 6 (d = 36)       pair 6  contour distance 2, pair 7: 3
      label 90: isolated."""
    lab = np.zeros((96, 96), np.uint32)
    put(lab, BOX, 2, 2, 11); put(lab, BOX, 2, 7, 12)
    put(lab, BOX, 2, 40, 21); put(lab, BOX, 7, 45, 22)
    put(lab, BOX, 30, 2, 31); put(lab, BOX, 30, 8, 32)
    put(lab, BOX, 30, 40, 41); put(lab, BOX, 30, 49, 42)
    put(lab, BOX, 58, 2, 51); put(lab, BOX, 58, 12, 52)
    put(lab, BOX, 58, 40, 61); put(lab, BOX, 58, 46, 62)
    put(lab, BOX, 80, 2, 71); put(lab, BOX, 80, 9, 72)
    put(lab, BOX, 84, 80, 90)
    return [lab]


def tiny():
    """A 1-pixel and a 2-pixel ROI (empty contours) against a disc, and a 3-pixel anti-diagonal: the pairs are skipped on both sides."""
    lab = np.zeros((48, 48), np.uint32)
    put(lab, disc(6), 10, 10, 5)
    put(lab, np.ones((1, 1), bool), 16, 23, 6)
    put(lab, np.ones((1, 2), bool), 9, 15, 7)
    put(lab, np.eye(3, dtype=bool)[::-1], 23, 21, 8)
    return [lab]


def corner():
    """One contour point (the corner of the box 1) adjacent to two neighbors (2 to its right, 3 above it): counted once.  Box 4 lies
    two pixels under box 1: a third neighbor."""
    lab = np.zeros((40, 40), np.uint32)
    put(lab, BOX, 10, 10, 1)
    put(lab, np.ones((3, 4), bool), 10, 15, 2)
    put(lab, np.ones((4, 3), bool), 6, 12, 3)
    put(lab, BOX, 17, 9, 4)
    return [lab]


def checker():
    """A bridged checkerboard (several sub-contours merged into one list) beside a box and a disc.  (The reference's tracer marks a pixel once:
    none of these inputs has a contour point twice.  The touch flags are per contour index whatever the list holds.)"""
    lab = np.zeros((40, 48), np.uint32)
    put(lab, checkerboard(), 8, 8, 3)
    put(lab, np.ones((9, 4), bool), 9, 21, 4)
    put(lab, disc(3), 21, 10, 9)
    return [lab]


def ties():
    """Label 5 between two equal boxes at bit-equal centroid distances (left: label 2, right: label 9; a third, label 12, above at the
    same distance): the lower label wins both minima.  A blob (label 20) inside a ring (label 21) with the same centroid: distance 0,
    angle 0."""
    lab = np.zeros((64, 64), np.uint32)
    put(lab, BOX, 10, 2, 2); put(lab, BOX, 10, 10, 5); put(lab, BOX, 10, 18, 9); put(lab, BOX, 2, 10, 12)
    put(lab, disc(12) & ~np.pad(disc(6), 6), 30, 30, 21)
    put(lab, disc(3), 39, 39, 20)
    return [lab]


def row4():
    """Four 3 x 3 blobs in a horizontal row: for the leftmost (at R = 12) three equal angles, the deviation exactly 0."""
    lab = np.zeros((24, 40), np.uint32)
    for k in range(4):
        put(lab, np.ones((3, 3), bool), 10, 4 + 4 * k, k + 1)
    return [lab]


def words():
    """Contours of 63 / 64 / 65 points (the wave's ballot word) beside each other, and one of 257 (one more than the workgroup)."""
    lab = np.zeros((96, 96), np.uint32)
    put(lab, box_bump(*WORD_BOXES[63]), 2, 2, 63)
    put(lab, box_bump(*WORD_BOXES[65]), 2, 5, 65)     # edge to edge with the 63-point box
    put(lab, box_bump(*WORD_BOXES[64]), 40, 2, 64)
    put(lab, disc(2), 46, 10, 7)
    lab2 = np.zeros((96, 96), np.uint32)
    put(lab2, box_bump(65, 65, 1), 2, 2, 257)
    put(lab2, disc(4), 30, 70, 3)
    put(lab2, np.ones((3, 20), bool), 70, 30, 4)
    return [lab, lab2]


def long_comb():
    """The 2641-point comb of circle_cases (beyond the LDS contour bound of the contour's other readers, several passes and several
    LDS tiles here) beside small ROIs."""
    lab = np.zeros((48, 176), np.uint32)
    put(lab, comb(40, 30, spine=2), 4, 4, 40)
    put(lab, disc(3), 38, 20, 41)
    put(lab, np.ones((3, 30), bool), 38, 60, 42)
    put(lab, disc(2), 10, 166, 43)
    put(lab, np.ones((2, 2), bool), 20, 10, 44)       # between two teeth
    return [lab]


def ring():
    """The 131 x 131 ring (a box beyond the LDS contour plane: the big-box chain) around and beside small ROIs."""
    lab = np.zeros((160, 160), np.uint32)
    put(lab, ring130(), 4, 4, 130)
    put(lab, disc(5), 64, 64, 1)                      # in the hole, far from the ring
    put(lab, disc(3), 66, 20, 2)                      # in the hole, near the ring's inner edge
    put(lab, disc(4), 60, 138, 3)                     # outside, near
    put(lab, np.ones((4, 4), bool), 150, 150, 4)      # outside, inside the ring's box corner
    return [lab]


def lattice():
    """A 20 x 20 lattice of 3 x 3 blobs, pitch 4: at R = 12 an inner blob has more candidates than a wave has lanes."""
    lab = np.zeros((80, 80), np.uint32)
    for i in range(20):
        for j in range(20):
            lab[4 * i:4 * i + 3, 4 * j:4 * j + 3] = 1 + 20 * i + j
    return [lab]


def three_images():
    """Three images with identical geometry and different labels (1..; non-contiguous 7 l + 3; 100000 + l)."""
    base = np.zeros((64, 64), np.uint32)
    rng = np.random.default_rng(77)
    lab_id = 0
    for gy in range(4):
        for gx in range(4):
            r = int(rng.integers(1, 6))
            lab_id += 1
            put(base, disc(r), 16 * gy + int(rng.integers(0, 16 - 2 * r)), 16 * gx + int(rng.integers(0, 16 - 2 * r)), lab_id)
    b = base.astype(np.int64)
    return [base, np.where(b > 0, 7 * b + 3, 0).astype(np.uint32), np.where(b > 0, 100000 + b, 0).astype(np.uint32)]


# name -> (builder, radii, origin)
CASES = {
    "contacts": (contacts, (1, 2, 5), None),
    "tiny": (tiny, (5,), None),
    "corner": (corner, (1, 2), None),
    "checker": (checker, (2, 5), None),
    "ties": (ties, (5,), None),
    "row4": (row4, (2, 12), None),
    "words": (words, (2, 5), None),
    "long_comb": (long_comb, (5,), None),
    "ring": (ring, (5, 12), None),
    "lattice": (lattice, (12,), None),
    "three_images": (three_images, (2, 5, 12), None),
    "placed": (contacts, (5,), (FAR_X, 5)),
}
API_CASE = "three_images"            # the stack behind api_expected.json


def images(name):
    return CASES[name][0]()


def intensity(lab, seed):
    return np.random.default_rng(seed).integers(1, 4096, lab.shape).astype(np.uint32)


def stack(name):
    """(I, M): the [n_images, H, W] stacks of the tile entry."""
    M = np.stack(images(name))
    I = np.stack([intensity(m, 500 + k) for k, m in enumerate(M)])
    return I, M


def batch_of_images(labs, origin=None, seed0=500) -> _abi.HostBatch:
    """The host batch of the batch entry: the ROIs of every image in ascending label order, image after image, with image_offset."""
    rois, off = [], [0]
    for k, lab in enumerate(labs):
        rr = synth.rois_from_tile(intensity(lab, seed0 + k), lab)
        if origin:
            rr = [dict(r, x=r["x"] + origin[0], y=r["y"] + origin[1]) for r in rr]
        rois += rr
        off.append(len(rois))
    b = _abi.batch_from_rois(rois)
    b.image_offset = np.asarray(off, np.uint64)
    return b


def batch(name) -> _abi.HostBatch:
    return batch_of_images(images(name), CASES[name][2])


def keys():
    return [(name, r) for name, (_, radii, _) in CASES.items() for r in radii]


def golden():
    """{(case, radius): (n_roi, 12) -- the nine columns, the contour length, CENTROID_X, CENTROID_Y -- as recorded from the
    reference's classes}."""
    with np.load(os.path.join(GOLDEN_DIR, "neighbors_reference.npz")) as z:
        return {(name, r): z[f"{name}__r{r}"] for name, r in keys()}


def api_expected():
    return json.load(open(os.path.join(GOLDEN_DIR, "api_expected.json")))
