"""Seeded inputs of the intensity-histogram tests (IH_* columns, nyxhip_ih_batch / nyxhip_ih_tiles) and the loader of the values recorded
from the reference's own IntensityHistogramFeatures (tests/golden/ih).  A case is a list of ROIs and the settings it runs under: the bin
count N (grey_depth) belongs to the call, not to the ROI."""
import json
import os

import numpy as np

from nyxus_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "ih")
SOFT_NAN = -7777.0
N_CAP = 4096                      # NYXHIP_ERR_UNSUPPORTED above it
WAVE_PX = 256                     # ROIs of at most this many pixels take the wave-per-ROI launch form


def published():
    """The two tables the reference's tests carry (tests/golden/ih/published.json): inputs and expected values."""
    return json.load(open(os.path.join(GOLDEN_DIR, "published.json")))


def line(values, label=1):
    v = np.asarray(values, np.uint32)
    return {"x": np.arange(len(v)), "y": np.zeros(len(v), np.int64), "inten": v, "label": label}


def block(values, width, label=1):
    v = np.asarray(values, np.uint32)
    i = np.arange(len(v))
    return {"x": i % width, "y": i // width, "inten": v, "label": label}


def ramp(lo, rng):
    """Every integer of [lo, lo + rng] once: every bin edge inside the range is met."""
    return line(np.arange(lo, lo + rng + 1, dtype=np.uint64))


def sampled_ramp(seed=5):
    """Range 2^32 - 2: the ends, the neighbours of every 64-bin edge and random values."""
    lo, hi, n = 1, 2 ** 32 - 1, 64
    bw = (float(hi) - float(lo)) / n
    vals = [lo, hi, lo + 1, hi - 1]
    for k in range(1, n):
        e = int(lo + k * bw)
        vals += [e - 1, e, e + 1, e + 2]
    rs = np.random.RandomState(seed)
    vals += rs.randint(lo, hi, 300, dtype=np.int64).tolist()
    return line(np.asarray(vals, np.uint64))


def sized(n, seed, hi=4096):
    rs = np.random.RandomState(seed)
    return block(rs.randint(1, hi, n), 32)


def flat_big():
    """300 x 300, flat but for two extreme pixels: one bin holds more than 65535 pixels."""
    v = np.full(300 * 300, 1000, np.uint32)
    v[17] = 10
    v[-5] = 5000
    return block(v, 300)


def disk(seed, hi, r=30):
    """The benchmark's ROI shape: a disk of radius 30 (2821 px)."""
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    m = xx * xx + yy * yy <= r * r
    rs = np.random.RandomState(seed)
    return {"x": xx[m] + r, "y": yy[m] + r, "inten": rs.randint(1, hi, int(m.sum())).astype(np.uint32)}


def _five():
    return [line(published()["five_pixel"]["intensities"])]


def _phantom():
    return [line(published()["ibsi_phantom"]["intensities"])]


def _gates():
    return [line([77]), line([500] * 40), line([9, 9])]                      # 1 px | a single intensity | 2 px of one intensity


def _two_px():
    return [line([3, 8])]


def _no_gradient():
    return [line([0, 0, 0, 1, 1]), line([4, 4, 9, 9]), line([1, 2, 2])]      # freq[1] < freq[0] | equal | the opposite, for contrast


def _sizes():
    return [sized(n, 100 + n) for n in (63, 64, 65, 255, 256, 257)] + [sized(700, 7, hi=65536)]


def _ramp64():
    return [ramp(5, 1), ramp(0, 1000), ramp(3, 65535), sampled_ramp()]


def _disks():
    return [disk(1, 4096), disk(2, 4096), disk(3, 65536), disk(4, 65536)]


def _mixed():
    rois = []
    for name in ("five", "phantom", "gates", "two_px", "no_gradient", "sizes", "ramp_n2", "ramp_n3", "ramp_n64", "ramp_n4096", "flat_big", "disks"):
        rois += CASES[name]["rois"]()
    return rois


# name -> {"rois": builder, "depth": N, "ibsi": 0 | 1, "soft_nan": value}
CASES = {
    "five": {"rois": _five, "depth": 3},
    "five_softnan": {"rois": _five, "depth": 3, "soft_nan": SOFT_NAN},
    "phantom": {"rois": _phantom, "depth": 6},
    "gates": {"rois": _gates, "depth": 64, "soft_nan": SOFT_NAN},
    "two_px": {"rois": _two_px, "depth": 2, "soft_nan": SOFT_NAN},
    "gate_negative_depth": {"rois": _sizes, "depth": -8, "soft_nan": SOFT_NAN},
    "gate_ibsi_off": {"rois": _sizes, "depth": 64, "ibsi": 0, "soft_nan": SOFT_NAN},
    "no_gradient": {"rois": _no_gradient, "depth": 2},
    "ramp_n2": {"rois": lambda: [ramp(7, 1)], "depth": 2},
    "ramp_n3": {"rois": lambda: [ramp(2, 7)], "depth": 3},
    "ramp_n64": {"rois": _ramp64, "depth": 64},
    "ramp_n4096": {"rois": lambda: [ramp(0, 65535)], "depth": N_CAP},
    "sizes": {"rois": _sizes, "depth": 64},
    "flat_big": {"rois": lambda: [flat_big()], "depth": 64},
    "disks": {"rois": _disks, "depth": 64},
    "mixed": {"rois": _mixed, "depth": 64, "soft_nan": SOFT_NAN},
}
# where the ROIs of the single cases that run at N = 64 lie in the mixed batch: name -> first row
MIXED_AT_64 = ("gates", "sizes", "ramp_n64", "flat_big", "disks")


def mixed_row(name):
    k = 0
    for other in ("five", "phantom", "gates", "two_px", "no_gradient", "sizes", "ramp_n2", "ramp_n3", "ramp_n64", "ramp_n4096", "flat_big", "disks"):
        if other == name:
            return k
        k += len(CASES[other]["rois"]())
    raise KeyError(name)


def settings(name):
    c = CASES[name]
    s = _abi.default_settings(64, bool(c.get("ibsi", 1)))
    s.grey_depth = int(c["depth"])
    s.soft_nan = float(c.get("soft_nan", 0.0))
    return s


_BATCHES = {}


def batch(name):
    if name not in _BATCHES:
        rois = [dict(r, label=k + 1) for k, r in enumerate(CASES[name]["rois"]())]
        _BATCHES[name] = _abi.batch_from_rois(rois)
    return _BATCHES[name]


# ---- the tile of the API fixture: a few ROIs of different sizes on one 96 x 96 uint16 image --------------------------------------------
API_DEPTH = 24


def api_tile():
    rs = np.random.RandomState(77)
    inten = rs.randint(1, 60000, (96, 96)).astype(np.uint16)
    lab = np.zeros((96, 96), np.uint16)
    lab[2:9, 3:10] = 3            # 49 px
    lab[12:30, 5:25] = 11         # 360 px
    lab[40:90, 30:90] = 7         # 3000 px
    lab[1, 60] = 40               # 1 px: gated
    lab[60:64, 2:6] = 21
    inten[60:64, 2:6] = 1234      # a single intensity: gated
    return inten, lab


def tile_batch():
    """The ROIs of api_tile() as a host batch, rows in label order."""
    inten, lab = api_tile()
    rois = []
    for v in sorted(int(u) for u in np.unique(lab) if u):
        xs, ys = np.nonzero(lab.T == v)                                      # column-major, the in-memory API's scan order
        rois.append({"x": xs, "y": ys, "inten": inten[ys, xs].astype(np.uint32), "label": v})
    return _abi.batch_from_rois(rois)


_GOLD = None


def golden():
    """name -> {"table": [n_roi x 46], "counts": list of per-ROI bin counts (empty for a gated ROI)}."""
    global _GOLD
    if _GOLD is None:
        z = np.load(os.path.join(GOLDEN_DIR, "ih_reference.npz"))
        _GOLD = {}
        for name in list(CASES) + ["tile"]:
            cnt, off = z[f"{name}__counts"], z[f"{name}__counts_offset"]
            _GOLD[name] = {"table": z[f"{name}__table"], "counts": [cnt[off[r]:off[r + 1]] for r in range(len(off) - 1)]}
    return _GOLD
