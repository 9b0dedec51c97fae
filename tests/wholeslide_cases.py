"""Seeded slides for the whole-slide tests (nyxhip_featurize_slides) and slide_batch(): the one-ROI-per-slide HostBatch whose rows the
entry must reproduce bit for bit -- the cloud is the slide in row-major order, the box is the image, the ROI's extrema and the slide's
extrema are those of all pixels (include/nyxhip.h, "whole-slide mode")."""
from __future__ import annotations

import zlib

import numpy as np

from nyxus_amd import _abi

# (w, h): the smallest slide of the largest size class; two co-occurrence strips and two slabs; single rows / columns (GLCM angles
# without a pair); a row length that is no multiple of 16; the largest class by pixel count alone; wider than a strip; two slides
# below the largest size class
SHAPES = [(257, 2), (257, 33), (1, 300), (300, 1), (259, 127), (181, 182), (8193, 5), (64, 64), (5, 4)]
DENSE_SHAPES = SHAPES[:7]
DTYPES = [np.uint8, np.uint16, np.uint32]
KLARGE_RANGE_MAX = 1 << 22                    # roi_kernel.h kLargeRangeMax: the histogram chain serves ranges below it


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def slide(w: int, h: int, dtype, kind: str = "random", seed: int = 0) -> np.ndarray:
    """One [h, w] slide.  kinds: random (the whole 8-bit range, 12 bits in the wider types, no zero), ibsi (1 .. 200), zeros (random with a
    third of the pixels zero), flat (all 7), allzero, range70000 and range4m (uint32: extrema 3 and 3 + 70000 / 3 + 2^22 + 5 present)."""
    r = _rng(w, h, np.dtype(dtype).name, kind, seed)
    top = 255 if np.dtype(dtype) == np.uint8 else 4095
    if kind == "random":
        a = r.integers(1, top + 1, (h, w))
    elif kind == "ibsi":
        a = r.integers(1, 201, (h, w))
    elif kind == "zeros":
        a = r.integers(1, top + 1, (h, w)) * (r.random((h, w)) > 0.33)
    elif kind == "flat":
        a = np.full((h, w), 7)
    elif kind == "allzero":
        a = np.zeros((h, w), np.int64)
    elif kind in ("range70000", "range4m"):
        span = 70000 if kind == "range70000" else KLARGE_RANGE_MAX + 5
        a = 3 + r.integers(0, span + 1, (h, w))
        a.flat[0] = 3
        a.flat[-1] = 3 + span
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a.astype(dtype))


def slide_batch(images) -> _abi.HostBatch:
    """The batch of section "whole-slide mode": ROI t is slide t -- pixels in row-major order (x = i % w, y = i / w, intensity widened to
    uint32), bbox = (w, h), min / max over all pixels, slide_min / slide_max the same two values as doubles, label 1."""
    offs, xs, ys, vs, bw, bh, mn, mx = [0], [], [], [], [], [], [], []
    for img in images:
        img = np.asarray(img)
        h, w = img.shape
        i = np.arange(w * h, dtype=np.int64)
        xs.append((i % w).astype(np.uint16))
        ys.append((i // w).astype(np.uint16))
        v = img.reshape(-1).astype(np.uint32)
        vs.append(v)
        bw.append(w); bh.append(h)
        mn.append(int(v.min())); mx.append(int(v.max()))
        offs.append(offs[-1] + w * h)
    n = len(bw)
    return _abi.HostBatch(np.ones(n, np.uint32), np.array(offs, np.uint64), np.concatenate(xs), np.concatenate(ys), np.concatenate(vs),
                          np.array(bw, np.uint32), np.array(bh, np.uint32), np.array(mn, np.uint32), np.array(mx, np.uint32),
                          np.array(mn, np.float64), np.array(mx, np.float64))


def settings(name: str) -> _abi.Settings:
    """gd8 / gd64 / gd300 (matlab binning), gdm16 (radiomics binning, 16 bins), ibsi, sub2 (GLCM angles 45 and 90 at offset 2, 64 levels)."""
    if name == "ibsi":
        return _abi.default_settings(64, True)
    if name == "sub2":
        s = _abi.default_settings(64)
        s.glcm_n_angles = 2
        s.glcm_angles[0] = 45
        s.glcm_angles[1] = 90
        s.glcm_offset = 2
        return s
    return _abi.default_settings({"gd8": 8, "gd64": 64, "gd300": 300, "gdm16": -16}[name])


# (settings, slide kind) of the invariant test; the last two exist as uint32 slides only
CASES = [("gd8", "random"), ("gd64", "random"), ("gdm16", "random"), ("ibsi", "ibsi"), ("gd300", "random"),
         ("gd64", "zeros"), ("gd64", "flat"), ("gd64", "allzero"), ("sub2", "random")]
CASES_U32 = [("gd64", "range70000"), ("gd64", "range4m")]


def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Element-wise: the same 64 bits, or NaN on both sides."""
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
