"""Seeded inputs of the image-quality tests (FOCUS_SCORE, LOCAL_FOCUS_SCORE, MAX_SATURATION, MIN_SATURATION: nyxhip_imq_batch / _tiles /
_slides) and the loader of the values recorded from the reference's own FocusScoreFeature and SaturationFeature (tests/golden/imq).
A case is a list of ROIs; every case but SIDE1 is recorded -- the reference's LOCAL_FOCUS_SCORE loop does not end on a box with a side of 1,
so such a box is never handed to it."""
import json
import os

import numpy as np

from nyxus_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "imq")
SOFT_NAN = -7777.0
NAMES = ["FOCUS_SCORE", "LOCAL_FOCUS_SCORE", "MAX_SATURATION", "MIN_SATURATION"]
WAVE_CELLS = 1024                 # kImqWaveCells: boxes of at most this many cells take the wave-per-ROI form
LDS_CELLS = 15360                 # kImqLdsCells: boxes of at most this many cells keep their plane in LDS


def published():
    """The 8 x 12 fixture of the reference's tests and its four published values (tests/golden/imq/published.json)."""
    return json.load(open(os.path.join(GOLDEN_DIR, "published.json")))


def filled(w, h, seed, hi=4096, lo=1):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return {"x": xx.ravel(), "y": yy.ravel(), "inten": rs.randint(lo, hi, w * h).astype(np.uint32)}


def masked(mask, seed, hi=4096):
    """The pixels of a boolean mask [h, w] with random non-zero intensities; the rest of the box is background."""
    rs = np.random.RandomState(seed)
    ys, xs = np.nonzero(mask)
    return {"x": xs, "y": ys, "inten": rs.randint(1, hi, len(xs)).astype(np.uint32)}


def disc(r, seed, hi=4096):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return masked(xx * xx + yy * yy <= r * r, seed, hi)


def ring(r, seed):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    d = xx * xx + yy * yy
    return masked((d <= r * r) & (d >= (r - 2) * (r - 2)), seed)


def comb(w, h, seed):
    m = np.zeros((h, w), bool)
    m[0, :] = True
    m[:, ::2] = True
    return masked(m, seed)


def _filled():
    return [filled(w, h, 10 * w + h) for w, h in ((2, 2), (2, 3), (3, 2), (3, 3), (5, 4), (4, 5), (7, 7))]


def _shapes():
    return [disc(6, 1), ring(9, 2), comb(11, 6, 3)]


def _flat():
    r = filled(6, 5, 0)
    r["inten"][:] = 777
    return [r]


def _zeros():
    r = filled(4, 3, 0)
    r["inten"][:] = 0
    return [r]


def _extreme():
    r = filled(6, 5, 0)
    r["inten"] = np.where((r["x"] + r["y"]) % 2 == 0, 2 ** 32 - 1, 0).astype(np.uint32)
    s = filled(5, 5, 4, hi=2 ** 32 - 1, lo=2 ** 31)
    s["inten"][7] = 0
    return [r, s]


def _widths():
    return [filled(w, 5, 200 + w, hi=65536) for w in (63, 64, 65)]


def _switches():
    # 32 x 32 = kImqWaveCells | 33 x 32: the workgroup form | 120 x 128 = kImqLdsCells | 121 x 127 = 15367: the global plane
    return [filled(32, 32, 31), filled(33, 32, 32, hi=65536), filled(120, 128, 33, hi=256), filled(121, 127, 34, hi=65536), disc(70, 35)]


def _published():
    p = published()
    a = np.asarray(p["image"], np.uint32)
    ys, xs = np.nonzero(a)                                                   # the 18 cells at 0 are background of the box
    return [{"x": xs, "y": ys, "inten": a[ys, xs]}]


def _side1():
    return [filled(1, 1, 1), filled(1, 5, 2), filled(5, 1, 3)]


CASES = {"published": _published, "filled": _filled, "shapes": _shapes, "flat": _flat, "zeros": _zeros, "extreme": _extreme, "widths": _widths,
         "switches": _switches}
SIDE1 = _side1
MIXED_ORDER = ("published", "filled", "shapes", "flat", "zeros", "extreme", "widths", "switches")


def settings():
    s = _abi.default_settings(256)
    s.soft_nan = SOFT_NAN
    return s


_BATCHES = {}


def batch(name):
    """The host batch of a case; "side1": the three side-1 boxes; "mixed": every recorded case in MIXED_ORDER, then the side-1 boxes."""
    if name not in _BATCHES:
        if name == "mixed":
            rois = [r for n in MIXED_ORDER for r in CASES[n]()] + SIDE1()
        else:
            rois = SIDE1() if name == "side1" else CASES[name]()
        _BATCHES[name] = _abi.batch_from_rois([dict(r, label=k + 1) for k, r in enumerate(rois)])
    return _BATCHES[name]


def mixed_row(name):
    k = 0
    for other in MIXED_ORDER:
        if other == name:
            return k
        k += len(CASES[other]())
    if name == "side1":
        return k
    raise KeyError(name)


# ---- the API fixture: two 64 x 80 uint16 tiles with a few ROIs each ---------------------------------------------------------------------
def api_tiles():
    rs = np.random.RandomState(91)
    inten = rs.randint(1, 60000, (2, 64, 80)).astype(np.uint16)
    lab = np.zeros((2, 64, 80), np.uint16)
    lab[0, 2:9, 3:10] = 3
    lab[0, 12:30, 5:26] = 11
    yy, xx = np.mgrid[0:64, 0:80]
    lab[0][(xx - 55) ** 2 + (yy - 40) ** 2 <= 15 ** 2] = 7
    lab[1, 5:50, 10:70] = 2
    lab[1, 55:60, 1:8] = 9
    inten[1, 55:60, 1:8] = 4321                                              # a flat ROI that fills its box
    inten[1, 20, 30] = 65535
    return inten, lab


def tile_batch():
    """The ROIs of api_tiles() as a host batch, rows in (tile, label) order."""
    inten, lab = api_tiles()
    rois = []
    for t in range(lab.shape[0]):
        for v in sorted(int(u) for u in np.unique(lab[t]) if u):
            ys, xs = np.nonzero(lab[t] == v)
            rois.append({"x": xs, "y": ys, "inten": inten[t][ys, xs].astype(np.uint32), "label": v})
    return _abi.batch_from_rois(rois)


def slide_batch(images):
    """The one-ROI-per-slide batch equivalent to a stack [n, H, W]: row-major clouds, the box is the image, extrema over all pixels."""
    rois = []
    for a in images:
        h, w = a.shape
        yy, xx = np.mgrid[0:h, 0:w]
        rois.append({"x": xx.ravel(), "y": yy.ravel(), "inten": a.ravel().astype(np.uint32)})
    return _abi.batch_from_rois(rois)


def slide(w, h, dtype, seed):
    rs = np.random.RandomState(seed)
    hi = min(int(np.iinfo(dtype).max), 2 ** 31)
    a = rs.randint(0, hi, (h, w)).astype(dtype)
    a[rs.randint(0, h), rs.randint(0, w)] = np.iinfo(dtype).max
    return a


_GOLD = None


def golden():
    """name -> recorded table [n_roi x 4] for every case of CASES, "tile" (tile_batch) and "slides" (the two api tiles as whole slides)."""
    global _GOLD
    if _GOLD is None:
        z = np.load(os.path.join(GOLDEN_DIR, "imq_reference.npz"))
        _GOLD = {k[:-len("__table")]: z[k] for k in z.files}
    return _GOLD
