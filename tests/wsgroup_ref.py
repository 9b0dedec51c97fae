"""numpy restatement of nyxhip_wsgroup_slides (include/nyxhip.h, "whole-slide mode: the rest of the *WHOLESLIDE* group"): the slide is
one ROI at origin (0, 0) in row-major order whose contour is its four corners K = (0,0), (w-1,0), (w-1,h-1), (0,h-1), each with the
slide's maximum as intensity.  tests/test_wsgroup_cpu.py pins it to the reference's tables (tests/golden/wsgroup); the GPU tests and
tools/wsgroup_fuzz.py use it where the reference does not exist.

Row layout: CONTOUR (7) | SMOMS (90) | IMOMS (90) | RADIAL (24), the blocks of nyxhip_wsgroup_slides in the order of the mask bits."""
import math

import numpy as np

from nyxus_amd import _abi
from tests import radial_ref

EPS_W = 0.001                                   # weighting_epsilon, 2d_geomoments_basic.h
BLOCKS = [(_abi.WS_CONTOUR, 7), (_abi.WS_SMOMS, 90), (_abi.WS_IMOMS, 90), (_abi.WS_RADIAL, 24)]
_PQ13 = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0)]
_PQ16 = [(p, q) for p in range(4) for q in range(4)]
_PQ7 = [(0, 2), (0, 3), (1, 1), (1, 2), (2, 0), (2, 1), (3, 0)]
_PQ10 = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (3, 0)]


def block_slice(mask: int, bit: int) -> slice:
    """Where the block of `bit` stands in a row of nyxhip_wsgroup_slides(mask)."""
    o = 0
    for b, n in BLOCKS:
        if b == bit:
            return slice(o, o + n)
        if mask & b:
            o += n
    raise ValueError(bit)


def corners(w, h):
    return np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.int64)


def contour_block(img):
    """ContourFeature::calculate over the four corners (contour.cpp:959-985): the perimeter closes K[3] -> K[0] first; Moments4 over
    four equal values has mean = the value and M2 = 0."""
    h, w = img.shape
    v = float(img.max())
    per = 0.0
    for s in (h - 1, w - 1, h - 1, w - 1):
        per += math.sqrt(float(s) * float(s))
    return np.array([per, per / math.pi, v, 0.0, v, v, ((v + v) + v) + v])


def weights(img, shape_variant: bool):
    """realintens of apply_dist2contour_weighting_wholeslide (2d_geomoments_basic.cpp:58-96), a vector<float>: epsilon for a pixel
    that shares its x or its y with a corner, else I * log(d + epsilon) with d = min(x, w-1-x, y, h-1-y)."""
    h, w = img.shape
    y, x = np.mgrid[0:h, 0:w]
    edge = (x == 0) | (x == w - 1) | (y == 0) | (y == h - 1)
    d = np.minimum(np.minimum(x, w - 1 - x), np.minimum(y, h - 1 - y)).astype(np.float64)
    inten = np.ones((h, w)) if shape_variant else img.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        wt = inten * np.log(d + EPS_W)
    wt = np.where(edge, EPS_W, wt)
    return wt.astype(np.float32).astype(np.float64)


def _hu(e):
    _02, _03, _11, _12, _20, _21, _30 = e
    a, b = _30 + _12, _21 + _03
    return [_20 + _02, (_20 - _02) ** 2 + 4 * _11 ** 2, (_30 - 3 * _12) ** 2 + (3 * _21 - _03) ** 2, a ** 2 + b ** 2,
            (_30 - 3 * _12) * a * (a ** 2 - 3 * b ** 2) + (3 * _21 - _03) * b * (3 * a ** 2 - b ** 2),
            (_20 - _02) * (a ** 2 - b ** 2) + 4 * _11 * a * b,
            (3 * _21 - _03) * a * (a ** 2 - 3 * b ** 2) - (_30 - 3 * _12) * b * (3 * a ** 2 - b ** 2)]


def moments_block(img, shape_variant: bool):
    """BasicGeomoms2D::calculate (2d_geomoments_basic.cpp:98-134) in whole-slide mode; 90 values in Feature2D order:
    RM(13) CM(16) NRM(16) NCM(7) HU(7) WRM(10) WCM(7) WNCM(7) WHU(7)."""
    h, w = img.shape
    y, x = np.mgrid[0:h, 0:w]
    x, y = x.astype(np.float64), y.astype(np.float64)
    inten = np.ones((h, w)) if shape_variant else img.astype(np.float64)

    def mom(wt, p, q, ox=0.0, oy=0.0):
        return float(np.sum(wt * (x - ox) ** p * (y - oy) ** q))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m00 = mom(inten, 0, 0)
        ox, oy = np.float64(mom(inten, 1, 0)) / m00, np.float64(mom(inten, 0, 1)) / m00
        rm = {pq: mom(inten, *pq) for pq in _PQ16}
        cm = {pq: mom(inten, pq[0], pq[1], ox, oy) for pq in _PQ16}
        nrm = [np.float64(rm[pq]) / np.float64(m00) ** ((pq[0] + pq[1]) / 2.0 + 1.0) for pq in _PQ16]
        ncm = [np.float64(cm[pq]) / np.float64(m00) ** ((pq[0] + pq[1]) / 2.0 + 1.0) for pq in _PQ7]
        wt = weights(img, shape_variant)
        w00 = mom(wt, 0, 0)
        wox, woy = np.float64(mom(wt, 1, 0)) / w00, np.float64(mom(wt, 0, 1)) / w00
        wrm = [mom(wt, *pq) for pq in _PQ10]
        wcm = [mom(wt, pq[0], pq[1], wox, woy) for pq in _PQ7]
        wncm = [np.float64(c) / np.float64(w00) ** ((pq[0] + pq[1]) / 2.0 + 1.0) for c, pq in zip(wcm, _PQ7)]
        out = [rm[pq] for pq in _PQ13] + [cm[pq] for pq in _PQ16] + nrm + ncm + _hu(ncm) + wrm + wcm + wncm + _hu(wncm)
    return np.array(out, np.float64)


def descents(x, y, K):
    """Pixel2::min_sqdist / max_sqdist v2 over FOUR points, by cases (pixel.cpp:40-70, :116-143): the first step is (int)(4 / log 4) = 2,
    so the first round compares corner 0 with corner 2 alone.  Corner 0 keeps a tie and ends the search; if corner 2 wins, the window
    becomes all four points and the second round walks corners 1, 2, 3 with step 1 (strict comparisons)."""
    d = [(K[i, 0] - x) ** 2 + (K[i, 1] - y) ** 2 for i in range(4)]
    mn = np.where(d[2] < d[0], np.minimum(np.minimum(d[1], d[2]), d[3]), d[0])
    mx = np.where(d[2] > d[0], np.maximum(np.maximum(d[1], d[2]), d[3]), d[0])
    return mn, mx


def centre(w, h):
    """find_center (pixel.cpp:146-162) over the row-major pixels: (index, max_sqdist of that pixel); the first pixel wins ties."""
    K = corners(w, h)
    i = np.arange(w * h, dtype=np.int64)
    x, y = i % w, i // w
    mn, mx = descents(x, y, K)
    o = int(np.argmin(mx - mn))                                  # first occurrence
    return o, int(mx[o])


def radial_block(img):
    """RadialDistributionFeature::calculate (radial_distribution.cpp:43-105) against the four corners; a centre with max_sqdist == 0
    (a 1 x 1 slide: undefined in the reference) gives 24 zeros."""
    h, w = img.shape
    n = radial_ref.NUM_BINS
    o, d2 = centre(w, h)
    if d2 == 0:
        return np.zeros(3 * n)
    i = np.arange(w * h, dtype=np.int64)
    x, y = i % w, i // w
    inten = img.reshape(-1).astype(np.int64)
    cx, cy = o % w, o // w
    dst_oc = math.sqrt(float(d2))
    dx, dy = x - cx, y - cy
    dst_oa = np.sqrt((dx * dx + dy * dy).astype(np.float64))
    bi = np.minimum(((dst_oa / dst_oc) * float(n - 1)).astype(np.int64), n - 1)
    ang = np.array([math.atan2(float(b_), float(a_)) for a_, b_ in zip(dx, dy)], np.float64)   # libm's atan2, like the reference
    ang = np.where(ang < 0, 2.0 * math.pi + ang, ang)
    w_bin = (ang / (2.0 * math.pi / float(n))).astype(np.int64)
    counts = np.bincount(bi, minlength=n)[:n]
    banded = np.zeros((n, n), np.int64)
    np.add.at(banded, (bi, w_bin), inten)
    out = np.zeros(3 * n)
    out[0:n] = counts.astype(np.float64) / (float(w * h) + radial_ref.EPSILON)
    out[n:2 * n] = banded.sum(axis=1).astype(np.float64) / (counts.astype(np.float64) + radial_ref.EPSILON)
    for r in range(n):
        s = 0.0
        for v in banded[r]:
            s += float(v)
        mean = s / float(n)
        s = 0.0
        for v in banded[r]:
            s += (float(v) - mean) * (float(v) - mean)
        out[2 * n + r] = math.sqrt(s / float(n)) / (mean + radial_ref.EPSILON)
    return out


def row(img, mask: int = _abi.WS_ALL) -> np.ndarray:
    parts = []
    if mask & _abi.WS_CONTOUR:
        parts.append(contour_block(img))
    if mask & _abi.WS_SMOMS:
        parts.append(moments_block(img, True))
    if mask & _abi.WS_IMOMS:
        parts.append(moments_block(img, False))
    if mask & _abi.WS_RADIAL:
        parts.append(radial_block(img))
    return np.concatenate(parts)


def table(images, mask: int = _abi.WS_ALL) -> np.ndarray:
    return np.stack([row(np.asarray(im), mask) for im in images])
