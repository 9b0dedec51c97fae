"""The inputs of the exact GLCM checks (tests/test_glcm_exact_cpu.py, tests/test_glcm_exact_gpu.py): small boxes, each the smallest at
which one form of the co-occurrence sweep still has its seam, combined pairwise across level tier x request x width x cloud order.

Groups (what the launch report can confirm stands in Case.sizes / workspace / coop; what it cannot is stated here):
  S  size class 0 (roi_small.hip; <= 256 px, sides <= 32, range < 2^14).  <= 8 levels: glcm_features_kernel8, two ROIs per wave;
     9..16: glcm_features_kernel, a wave per ROI; 17..64: the pair form with byte cells, distance 1 only -- offsets 2 / 3 at those
     levels leave it, which the report does not show (both are size class 0).
  W  classes 1-2 at <= 16 levels: the exported-count block of roi_features.hip.  Width 129 is the first box of size class 3.  The two
     "cloud" cases: INTENSITY + GLCM overlaps the sweep with the order statistics only while 16 (Ng + 1)^2 bytes of matrices fit the
     value buffer (2 bytes x the class's pixel count rounded up to a power of two): 16 levels beside 300-pixel clouds does not
     (serial order), 8 levels beside 700-pixel clouds does.  The report does not tell the two orders apart.
  G  classes 1-2 at 17..64 levels: 16-bit cells.  Largest box of the class < 48 x 48 cells: four waves; GLCM alone and a box
     >= 48 x 48: eight waves; an ROI with intensities up to 2^20 (range >= 65536) cannot use the 16-bit tables: the generic
     tiers (under INTENSITY + GLCM the report shows it as a wide-range class of its own).  Not in the report either.  The capacity case: 128 x 128 full, almost flat, symmetric -- one cell holds 2 x 16 256.
  D  65..180 levels: deep matrices, 4 -> 2 -> 1 angles per pass; in LDS up to 128 levels, at 180 the report names the workspace.  IBSI
     with a largest intensity above 128 is served with the large ROIs.
  X  255 / 256 levels and IBSI with largest intensity 1000: matrices in the global workspace or the large-ROI path.
  L  size classes 3-4 (roi_large.hip; the report lists them as one group under the larger class): strips of 8192 cells (rps = 8192 // w rows), column strips of 62 centres, thin boxes whose
     every row is a strip of its own, clouds in row-major (plane as is) and column-major order (transposed plane).
  T  the dense loader (featurize_slides_host) and the window loader (featurize_tiles_host), one case each.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

from nyxus_amd import _abi
from tests import glcm_exact_ref as gx
from tests.test_texture_counts_gpu import seam_roi

REQUESTS = {                      # name -> (angles, offset, symmetric)
    "usual": ((0, 45, 90, 135), 1, 0),
    "sym": ((0, 45, 90, 135), 1, 1),
    "a135": ((135,), 1, 0),
    "a45_135": ((45, 135), 1, 0),
    "a0_45_90": ((0, 45, 90), 1, 0),
    "off2": ((0, 45, 90, 135), 2, 0),
    "off3": ((0, 45, 90, 135), 3, 0),
}
SEAM_KINDS = ("columns", "shifted_runs", "diag45", "diag135", "seam_holes", "serpentine", "checker", "noise")
KINDS = SEAM_KINDS + ("zero_seams", "almost_flat")
STRIP_CELLS = 8192                # kLtexCells / the strips of roi_large.hip
_DRAWN = ("noise", "seam_holes", "zero_seams", "hole3", "wide20")     # the kinds whose content comes from the generator


def settings(gd, ibsi, request, soft_nan=0.0):
    s = _abi.default_settings(gd if not ibsi else 8, bool(ibsi))
    angles, off, sym = REQUESTS[request]
    s.glcm_n_angles = len(angles)
    for i, a in enumerate(angles):
        s.glcm_angles[i] = a
    s.glcm_offset, s.glcm_symmetric, s.soft_nan = off, sym, soft_nan
    return s


def roi(w, h, kind, rng, hi=4096, rows=None, order="col"):
    """A w x h box of one content kind with intensities in [1, hi), the value hi - 1 present.  rows: rows per strip, where the seams
    lie (default: the strips of roi_large.hip).  order: the cloud in column-major ('col', the scan order) or row-major order."""
    r = rows if rows is not None else max(1, STRIP_CELLS // w)
    if kind == "wide20":                                         # intensities up to 2^20: the range rules the 16-bit tables out
        kind, hi = "noise", 1 << 20
    if kind == "hole3":                                          # noise with the centre of the box missing
        yy, xx = np.mgrid[0:h, 0:w]
        keep = ~((yy == h // 2) & (xx == w // 2))
        v = rng.integers(1, hi, (h, w))
        v[0, 0] = hi - 1
        d = dict(x=xx.T[keep.T], y=yy.T[keep.T], inten=v.T[keep.T].astype(np.uint32))
    elif kind == "almost_flat":                                    # one value everywhere, one corner pixel at the maximum
        yy, xx = np.mgrid[0:h, 0:w]
        v = np.full((h, w), max(1, hi // 7), np.int64)
        v[h - 1, w - 1] = hi - 1
        d = dict(x=xx.T.ravel(), y=yy.T.ravel(), inten=v.T.ravel().astype(np.uint32))
    elif kind == "zero_seams":                                   # zero intensities on columns 61..66 and on the rows either side of every seam
        yy, xx = np.mgrid[0:h, 0:w]
        v = rng.integers(1, hi, (h, w))
        zero = ((xx >= 61) & (xx <= 66)) | (((yy % r) == 0) | ((yy % r) == r - 1)) & (yy > 0) & (yy < h - 1)
        v[zero & (rng.random((h, w)) < 0.5)] = 0
        v[0, 0] = hi - 1
        d = dict(x=xx.T.ravel(), y=yy.T.ravel(), inten=v.T.ravel().astype(np.uint32))
    else:
        d = seam_roi(w, h, r, kind, rng, hi=hi)
        # the largest intensity is hi - 1 whatever the kind, on the pixel in the middle of the box when the cloud has it: a pixel that
        # takes part in pairs of every angle (a checkerboard's diagonal pairs are otherwise split evenly between two cells, and every
        # column of the sensitivity condition is an integer)
        mid = np.nonzero((d["x"] == w // 2) & (d["y"] == h // 2))[0]
        d["inten"][mid[0] if len(mid) else 0] = hi - 1
        left = np.nonzero((d["x"] == w // 2 - 1) & (d["y"] == h // 2))[0]     # ... and a third value beside it (two-valued kinds)
        if len(left) and kind not in _DRAWN:
            d["inten"][left[0]] = 1 + hi // 2
    if order == "row":
        o = np.lexsort((d["x"], d["y"]))
        d = dict(x=d["x"][o], y=d["y"][o], inten=d["inten"][o])
    return d


@dataclass
class Case:
    group: str
    name: str
    gd: int
    ibsi: bool
    request: str
    boxes: tuple                  # ((w, h, kind[, order]), ...)
    hi: int = 4096
    rows: Optional[int] = None    # rows per "strip" of the content kinds (small boxes: a few rows)
    sizes: tuple = ()             # size classes the launch report may name for this call ((): not asserted)
    workspace: Optional[bool] = None   # bit 0 of "workspace" set on some launch of the call
    coop: Optional[bool] = None        # bit 0 of "cooperative" set on every launch of the call
    seed: int = 0

    @property
    def id(self):
        return "%s-%s-%s-%s" % (self.group, self.name, ("ibsi%d" % (self.hi - 1)) if self.ibsi else "gd%d" % self.gd, self.request)

    def settings(self, soft_nan=0.0):
        return settings(self.gd, self.ibsi, self.request, soft_nan)


@functools.lru_cache(maxsize=None)
def _rois(i):
    """The case's ROIs.  An ROI with drawn content that misses the sensitivity condition under the case's settings (a 2 x 2 box whose
    two pairs happen to give integer means) is drawn again, up to 40 times: the condition is computed from the exact reference
    alone, so this selects inputs, never outputs.  What still misses it fails test_every_case_is_sensitive_to_one_pair."""
    c = CASES[i]
    rng = np.random.default_rng(1000 + 7 * i + c.seed)
    s = c.settings()
    rois = []
    for bx in c.boxes:
        for _ in range(40):
            d = roi(bx[0], bx[1], bx[2], rng, hi=c.hi, rows=c.rows, order=bx[3] if len(bx) > 3 else "col")
            if bx[2] not in _DRAWN or bx[0] * bx[1] > 64:
                break
            e = gx.exact_glcm(_abi.batch_from_rois([d]), 0, s)
            if e.degenerate or min(gx.sensitivity(e)) >= 1000:
                break
        rois.append(d)
    return tuple(rois)


@functools.lru_cache(maxsize=None)
def _batch(i):
    return _abi.batch_from_rois(_rois(i))


def rois(c: Case):
    """The case's ROIs as dicts (shared: do not modify)."""
    return _rois(CASES.index(c))


def batch(c: Case) -> _abi.HostBatch:
    return _batch(CASES.index(c))


@functools.lru_cache(maxsize=None)
def _exact(i, soft_nan):
    c = CASES[i]
    b, s = _batch(i), c.settings(soft_nan)
    return tuple(gx.exact_glcm(b, r, s) for r in range(b.n_roi))


def exact(c: Case, soft_nan=0.0):
    """exact_glcm of every row of the case's batch (computed once per process)."""
    return _exact(CASES.index(c), soft_nan)


# ---- the lattice ------------------------------------------------------------------------------------------------------------

def _cycle(boxes, kinds, shift=0):
    return tuple((w, h, kinds[(i + shift) % len(kinds)]) + tuple(rest) for i, (w, h, *rest) in enumerate(boxes))


_S_BOXES = ((2, 1), (1, 2), (32, 1), (1, 32), (2, 2), (16, 16), (8, 32), (32, 8), (16, 16), (13, 11), (32, 8), (8, 32), (16, 16))
_S_KINDS = ("noise", "noise", "noise", "noise", "noise", "noise", "diag45", "noise", "checker", "seam_holes", "almost_flat", "almost_flat", "almost_flat")


def _s_case(gd, request, k):
    boxes = tuple((w, h, kind) for (w, h), kind in zip(_S_BOXES, _S_KINDS)) + ((3, 3, "hole3"), (5, 3, "hole3"))
    return Case("S", "small", gd, False, request, boxes, rows=4, sizes=(0,), workspace=False, coop=False, seed=k)


# widths around a wave and two waves x the heights where a wave of the row split gets no row (floor(h c / 20)), 20 / 21, 61
_W_BOXES = ((1, 61), (2, 61), (63, 1), (64, 2), (65, 3), (66, 4), (127, 5), (128, 6), (63, 21), (64, 61), (65, 20), (66, 21), (127, 61), (128, 20))
_W3_BOXES = ((129, 20), (129, 3), (129, 61))          # the first width of size class 3


def _w_case(gd, request, k):
    # (two-valued kinds on boxes a few rows high: at offsets 2 / 3 the rows that hold the odd pixels pair with nothing, and the means are integers)
    kinds = KINDS if request not in ("off2", "off3") else tuple(x for x in KINDS if x not in ("checker", "serpentine"))
    return Case("W", "widths", gd, False, request, _cycle(_W_BOXES, kinds, k), rows=5, sizes=(0, 1, 2), workspace=False, coop=False, seed=k)


_G4_BOXES = ((47, 47), (33, 40), (40, 33), (1, 47), (47, 1), (2, 40), (47, 3), (20, 21))                      # every box < 48 x 48 cells: four waves
_G8_BOXES = ((63, 21), (64, 61), (65, 20), (66, 5), (127, 61), (128, 20), (128, 61), (48, 48), (127, 3), (65, 61), (1, 61), (2, 61))


_D_BOXES = ((20, 20), (70, 40), (20, 20), (70, 40), (20, 20), (64, 5))
_X_BOXES = ((24, 24), (24, 24), (24, 24), (129, 4))


def _rps(w):
    return STRIP_CELLS // w


def _l_boxes(k, thin, kinds=KINDS):
    """Five widths (three column strips of exactly 62 at 186; four and more from 249), each with one of the heights 2 rps - 1, 2 rps,
    2 rps + 1 (which one rotates with k), every box once with a column-major and once with a row-major cloud; plus thin boxes."""
    out = []
    for i, w in enumerate((129, 186, 187, 248, 249)):
        h = 2 * _rps(w) - 1 + (i + k) % 3
        kind = kinds[(2 * i + 3 * k) % len(kinds)]
        out += [(w, h, kind, "col"), (w, h, kind, "row")]
    for j, (w, h) in enumerate(thin):
        kind = ("noise", "zero_seams", "columns", "diag135")[(j + k) % 4]
        out += [(w, h, kind, "col"), (w, h, kind, "row")]
    return tuple(out)


def _build():
    C = []
    # S: levels 3 / 8 (kernel8), 9 / 16 (kernel), 17 / 33 / 64 (pair form; offsets 2 / 3 leave it)
    for k, (gd, req) in enumerate([(3, "usual"), (3, "a45_135"), (8, "usual"), (8, "sym"), (8, "off2"), (9, "a135"), (16, "sym"), (16, "off3"), (17, "usual"),
                                   (17, "sym"), (17, "off2"), (33, "a45_135"), (64, "usual"), (64, "sym"), (64, "off3"), (64, "a0_45_90")]):
        C.append(_s_case(gd, req, k))
    # W: every request at 8 and at 16 levels
    for k, req in enumerate(REQUESTS):
        C.append(_w_case(8, req, k))
        C.append(_w_case(16, req, k + 5))
    C.append(Case("W", "w129", 8, False, "usual", _cycle(_W3_BOXES, KINDS, 1), rows=5, sizes=(3,), coop=True))
    C.append(Case("W", "w129", 16, False, "sym", _cycle(_W3_BOXES, KINDS, 4), rows=5, sizes=(3,), coop=True))
    C.append(Case("W", "cloud300", 16, False, "usual", _cycle(((20, 15), (15, 20), (20, 15)), KINDS, 2), rows=5, sizes=(1,), workspace=False, coop=False))
    C.append(Case("W", "cloud700", 8, False, "usual", _cycle(((35, 20), (20, 35), (35, 20)), KINDS, 5), rows=5, sizes=(1,), workspace=False, coop=False))
    # G: 17 / 33 / 64 levels, four waves, eight waves, the fall-back, the capacity case
    for k, (gd, req) in enumerate([(17, "usual"), (33, "sym"), (64, "usual"), (64, "a135"), (64, "off2")]):
        C.append(Case("G", "four_wave", gd, False, req, _cycle(_G4_BOXES, KINDS, k), rows=5, sizes=(0, 1), workspace=False, coop=False, seed=k))
    for k, (gd, req) in enumerate([(17, "sym"), (33, "usual"), (33, "off3"), (64, "usual"), (64, "sym"), (64, "a0_45_90")]):
        C.append(Case("G", "eight_wave", gd, False, req, _cycle(_G8_BOXES, KINDS, k), rows=5, sizes=(0, 1, 2), workspace=False, coop=False, seed=k))
    C.append(Case("G", "wide_range", 64, False, "usual", _cycle(((40, 33), (33, 40)), KINDS, 0) + ((40, 33, "wide20"),), rows=5, sizes=(1,), coop=False))
    C.append(Case("G", "wide_range", 33, False, "sym", _cycle(((40, 33), (33, 40)), KINDS, 3) + ((33, 40, "wide20"),), rows=5, sizes=(1,), coop=False))
    C.append(Case("G", "capacity", 64, False, "sym", ((128, 128, "almost_flat"),), sizes=(2,), workspace=False, coop=False))
    C.append(Case("G", "capacity", 64, False, "usual", ((128, 128, "almost_flat"), (128, 128, "checker")), sizes=(2,), workspace=False, coop=False))
    # D: deep matrices in LDS
    for k, (gd, req) in enumerate([(65, "usual"), (90, "sym"), (128, "usual"), (128, "a45_135"), (180, "usual"), (180, "off2"), (90, "a0_45_90")]):
        ws = gd > 128                                   # (180 levels: the launch report names the workspace, not LDS)
        C.append(Case("D", "deep", gd, False, req, _cycle(_D_BOXES, KINDS, k), rows=5, sizes=(1, 2), workspace=ws, coop=None if ws else False, seed=k))
    C.append(Case("D", "deep", 0, True, "usual", _cycle(_D_BOXES, KINDS, 1), hi=101, rows=5, sizes=(1, 2), workspace=False, coop=False))
    C.append(Case("D", "deep", 0, True, "a135", _cycle(_D_BOXES, KINDS, 2), hi=201, rows=5, sizes=(3,)))
    # X: matrices beyond LDS
    for k, (gd, req) in enumerate([(255, "usual"), (256, "sym"), (256, "off3")]):
        C.append(Case("X", "workspace", gd, False, req, _cycle(_X_BOXES, KINDS, k), rows=5, workspace=True, seed=k))
    C.append(Case("X", "workspace", 0, True, "usual", _cycle(_X_BOXES, KINDS, 4), hi=1001, rows=5, sizes=(3,)))
    C.append(Case("X", "workspace", 0, True, "a45_135", _cycle(_X_BOXES, KINDS, 6), hi=1001, rows=5, sizes=(3,)))
    # L: the large-ROI path; levels 8 (matrices in LDS), 100 (counted in place in the workspace), 300 (16-bit plane), -16 (level map), IBSI
    thin = ((4100, 3), (2800, 5))
    for k, (gd, ibsi, req, th) in enumerate([(8, 0, "usual", thin), (8, 0, "sym", thin), (8, 0, "a135", thin), (8, 0, "off2", thin + ((20000, 3),)),
                                             (100, 0, "usual", thin), (100, 0, "a45_135", thin), (100, 0, "off3", thin), (300, 0, "sym", thin),
                                             (300, 0, "a0_45_90", thin), (-16, 0, "usual", thin), (-16, 0, "off2", thin),
                                             (0, 1, "usual", thin + ((20000, 3),)), (0, 1, "sym", thin)]):
        # (two of 100 or 300 levels on 16 000 pixels: means within a few 1 / N of integers, too little for the sensitivity condition)
        kinds = KINDS if gd in (8, -16) or ibsi else tuple(x for x in KINDS if x not in ("checker", "serpentine", "almost_flat"))
        C.append(Case("L", "large", gd, bool(ibsi), req, _l_boxes(k, th, kinds), hi=61 if ibsi else 4096, sizes=(3, 4), coop=True, seed=k))
    return C


CASES = _build()
GROUPS = ("S", "W", "G", "D", "X", "L")


def of_group(g):
    return [c for c in CASES if c.group == g]


# ---- T: the other entries ---------------------------------------------------------------------------------------------------

def slide(dtype, seed=0):
    """A 130 x 129 slide (width 130: past two waves; height 129) with zeros scattered in."""
    rng = np.random.default_rng(seed)
    hi = 256 if dtype == np.uint8 else 4096
    a = rng.integers(1, hi, (129, 130))
    a[rng.random(a.shape) < 0.03] = 0
    a[0, 0] = hi - 1
    return a.astype(dtype)


def slide_batch(img):
    h, w = img.shape
    yy, xx = np.mgrid[0:h, 0:w]
    return _abi.batch_from_rois([dict(x=xx.ravel(), y=yy.ravel(), inten=img.ravel().astype(np.uint32))])


def tile96(seed=0):
    """One 96 x 96 tile with four ROIs (labels 3, 5, 9, 12): a 40 x 33 block, a 33 x 40 block, a disc and an L shape."""
    rng = np.random.default_rng(seed)
    inten = rng.integers(1, 4096, (96, 96)).astype(np.uint32)
    lab = np.zeros((96, 96), np.uint32)
    lab[2:35, 3:43] = 3
    lab[40:80, 1:34] = 5
    yy, xx = np.mgrid[0:96, 0:96]
    lab[(xx - 70) ** 2 + (yy - 22) ** 2 <= 18 ** 2] = 9
    lab[50:94, 45:60] = 12
    lab[80:94, 45:94] = 12
    return inten, lab
