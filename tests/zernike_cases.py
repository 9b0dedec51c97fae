"""TEST INFRASTRUCTURE -- deterministic ZERNIKE2D inputs for tests/test_zernike_cpu.py and tests/test_zernike_gpu.py, at the places where
a moment kernel goes wrong without a blanket 1e-5 noticing: pixels within an ulp (and within 1e-12) of the unit-disc test, a centroid on a
pixel, boxes that leave the disc nearly empty, cloud sizes at every stride tail and at the LDS staging cap, and clouds whose high-order
moments are large.  Every ROI is one named case; tests/golden/zernike/zernike_exact.json holds its 30 exact magnitudes
(tests/zernike_ref.exact), written once by tests/golden/zernike/make_zernike_golden.py.

a. edge    full (2N + 1) x N and N x (2N + 1) rectangles with point-symmetric intensities (the centroid is the exact centre), so the
           lattice points with dx^2 + dy^2 = N^2 lie ON the circle; one pixel raised by t slides the centroid by t d / m00 and walks those
           pixels through the last ulps and through the kernel's 1e-12 redo band.  EDGE_KEPT is the outcome of search_edge().
b. centre  the centroid on a pixel (r == 0, dropped), the smallest positive r the family reaches, r on both sides of 1e-12.
c. aspect  1 x k, k x 1, 2 x 65, 65 x 2, an empty disc, an L and a ring.
d. sizes   ragged clouds of 2 .. 4099 pixels, zeros among the intensities, and the companions that set the launch form and the cap.
e. coeff   thin rings and a two-point dumbbell: every one of the 30 columns is above 1e-3 somewhere.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

from nyxus_amd import _abi
from tests import zernike_ref as zr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zernike", "zernike_exact.json")
EDGE_N = (13, 17, 25, 65)
MODES = ("u8", "u16", "u32")


def _mix(k, salt):
    """A fixed integer hash, 31 bits (wrapping 64-bit arithmetic)."""
    k = np.asarray(k, np.uint64)
    with np.errstate(over="ignore"):
        z = k * np.uint64(6364136223846793005) + np.uint64(salt) * np.uint64(1442695040888963407) + np.uint64(1)
        z ^= z >> np.uint64(29)
        z = z * np.uint64(0xBF58476D1CE4E5B9)
    return ((z >> np.uint64(33)) & np.uint64(0x7FFFFFFF)).astype(np.int64)


def _roi(x, y, v):
    x = np.asarray(x, np.int64)
    y = np.asarray(y, np.int64)
    assert x.min() == 0 and y.min() == 0 and len(x) == len(y) == len(v)
    return {"x": x, "y": y, "inten": np.asarray(v, np.uint32)}


def box(roi):
    return int(roi["x"].max()) + 1, int(roi["y"].max()) + 1


def members(roi):
    w, h = box(roi)
    return zr.members(roi["x"], roi["y"], roi["inten"], w, h)


# ---- a. the disc edge ---------------------------------------------------------------------------------------------------------------------
_MODE = {"u8": (1, 200, 255), "u16": (1000, 59000, 65535), "u32": (2 ** 31, 2 ** 31 - 2 ** 25, 2 ** 32 - 1)}   # (floor, span, the edge pixels)


def edge_offsets(N, transposed):
    """The lattice points on the circle of radius N inside the box, as offsets from the centre."""
    hw, hh = (N // 2, N) if transposed else (N, N // 2)
    return [(dx, dy) for dx in range(-hw, hw + 1) for dy in range(-hh, hh + 1) if dx * dx + dy * dy == N * N]


def edge_case(N, transposed, mode, a=0, b=0, t=0):
    """The full rectangle, point-symmetric intensities, the on-circle pixels brightest; the pixel at offset (a, b) raised by t."""
    w, h = (N, 2 * N + 1) if transposed else (2 * N + 1, N)
    cx, cy = (w - 1) // 2, (h - 1) // 2
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    x, y = x.ravel(), y.ravel()
    dx, dy = x - cx, y - cy
    flip = (dx < 0) | ((dx == 0) & (dy < 0))                                 # one key for p and -p
    key = np.where(flip, -dx, dx) * 1024 + np.where(flip, -dy, dy) + 512
    lo, span, top = _MODE[mode]
    v = lo + _mix(key, N) % span
    v[dx * dx + dy * dy == N * N] = top
    if t:
        assert (a, b) not in edge_offsets(N, transposed)
        k = int(np.flatnonzero((dx == a) & (dy == b))[0])
        v[k] += t
        assert v[k] < top
    return _roi(x, y, v)


def edge_pixels(roi, N, transposed):
    """(offset, cloud index) of the on-circle pixels."""
    w, h = box(roi)
    cx, cy = (w - 1) // 2, (h - 1) // 2
    return [((dx, dy), int(np.flatnonzero((roi["x"] == cx + dx) & (roi["y"] == cy + dy))[0])) for dx, dy in edge_offsets(N, transposed)]


CATEGORIES = ("r2_one", "r2_one_ulp", "r2_above", "r2_below", "in_band_below", "in_band_above", "off_band_below", "off_band_above")
FLIPS = ("flip_fma_xx", "flip_fma_yy")                                       # fma(x, x, y * y) / fma(y, y, x * x) decides the other way
ULP = 2.0 ** -52


def classify(r2, r):
    """The categories one edge pixel's double r2, r fall in."""
    out = []
    if r2 == 1.0: out.append("r2_one")
    if r2 == 1.0 + ULP: out.append("r2_one_ulp")
    if 1.0 + 2 * ULP <= r2 <= 1.0 + 8 * ULP: out.append("r2_above")
    if 1.0 - 4 * ULP <= r2 < 1.0: out.append("r2_below")
    d = abs(r - 1.0)
    side = "below" if r < 1.0 else "above"
    if 2.5e-13 < d < 1e-12: out.append("in_band_" + side)
    if 1e-12 < d < 4e-12: out.append("off_band_" + side)
    return out


def edge_census(roi, N, transposed):
    """{category: count} over the on-circle pixels of one case, the decision checked against the category on the way."""
    mem = members(roi)
    count = {c: 0 for c in CATEGORIES + FLIPS}
    for _, k in edge_pixels(roi, N, transposed):
        r2, r, kept = float(mem["r2"][k]), float(mem["r"][k]), bool(mem["keep"][k])
        cats = classify(r2, r)
        for c in cats:
            count[c] += 1
            assert kept == (c in ("r2_one", "r2_one_ulp", "r2_below", "in_band_below", "off_band_below")), (c, r2, r, kept)
        fa, fb = zr.r2_fused(mem["X"][k], mem["Y"][k])
        count["flip_fma_xx"] += zr.decision(fa) != kept
        count["flip_fma_yy"] += zr.decision(fb) != kept
    return count


def _edge_probe(N, transposed, mode):
    """A family's on-circle pixels without building its members: t -> (X, Y, r2, r) of those pixels, from the base's sums."""
    base = edge_case(N, transposed, mode)
    w, h = box(base)
    cx0, cy0 = (w - 1) // 2, (h - 1) // 2
    mem = members(base)
    ex = np.array([cx0 + dx + 1.0 for dx, _ in edge_offsets(N, transposed)])
    ey = np.array([cy0 + dy + 1.0 for _, dy in edge_offsets(N, transposed)])

    def at(a, b, t):
        m00 = mem["sum"] + t
        X = (ex - (mem["m10"] + t * (cx0 + a + 1)) / m00) / float(N)
        Y = (ey - (mem["m01"] + t * (cy0 + b + 1)) / m00) / float(N)
        xx, yy = X * X, Y * Y
        r2 = xx + yy
        return X, Y, r2, np.sqrt(r2)
    return at


def search_edge(want=6, per_base=3):
    """The CPU search whose outcome EDGE_KEPT records (run by hand when the bases change; about a minute).  A family raises the pixel at
    offset (a, b) of a base by t.  Pass 1, N = 65 at 32 bits (a step of t moves r2 by less than an ulp), every t below 600: members with an
    on-circle pixel that a fused x * x + y * y decides the other way.  Pass 2, t = 1, 2, 4, ...: a member is kept while it adds an
    on-circle pixel to a category still short of `want`, at most `per_base` per base.  Pass 3, the other widths and sizes: per base the
    first members with two or more pixels in the bands around 1e-12."""
    have = {c: 0 for c in CATEGORIES + FLIPS}
    kept = []

    def keep(k):
        c = edge_census(edge_case(*k), k[0], k[1])
        kept.append(k)
        for q in c:
            have[q] += c[q]
    offsets = lambda reach: [(a, b) for a in range(-reach, reach + 1) for b in range(-reach, reach + 1) if (a, b) != (0, 0)]
    for tr in (False, True):
        at, n = _edge_probe(65, tr, "u32"), 0
        for a, b in offsets(6):
            for t in range(1, 600):
                if n >= per_base:
                    break
                X, Y, r2, _ = at(a, b, t)
                for k in np.flatnonzero(np.abs(r2 - 1.0) < 1e-14):
                    if any(zr.decision(f) != zr.decision(float(r2[k])) for f in zr.r2_fused(X[k], Y[k])):
                        c = edge_census(edge_case(65, tr, "u32", a, b, t), 65, tr)
                        if any(c[q] and have[q] < per_base for q in FLIPS):
                            keep((65, tr, "u32", a, b, t))
                            n += 1
                        break
    fine = [c for c in CATEGORIES if c not in ("r2_one", "r2_one_ulp")]       # (those two: the bases themselves)
    for N, tr, mode in [(65, False, "u32"), (65, True, "u32")]:
        at, n = _edge_probe(N, tr, mode), 0
        for a, b in offsets(4):
            t = 1
            while t <= 2 ** 22 and n < per_base:
                _, _, r2, r = at(a, b, t)
                cats = {c for q in range(len(r)) for c in classify(float(r2[q]), float(r[q]))}
                if any(have[c] < want for c in cats if c in fine):
                    keep((N, tr, mode, a, b, t))
                    n += 1
                t *= 2
    for N, tr, mode in [(65, False, "u16"), (65, True, "u16"), (25, False, "u32"), (25, True, "u32"), (17, True, "u32"), (13, False, "u32")]:
        n = 0
        for a, b in offsets(4):
            t = 1
            while t <= (2 ** 22 if mode == "u32" else 4096) and n < 2:       # (the raised pixel stays below the on-circle pixels)
                c = edge_census(edge_case(N, tr, mode, a, b, t), N, tr)
                if sum(c[q] for q in c if "band" in q) >= 2:
                    keep((N, tr, mode, a, b, t))
                    n += 1
                t *= 2
    return kept, have


# (N, transposed, mode, a, b, t): the members of the families that search_edge() kept
EDGE_KEPT = [(65, False, "u32", -2, -5, 5), (65, False, "u32", -2, 5, 5), (65, False, "u32", -1, -4, 29),
             (65, True, "u32", -5, -2, 5), (65, True, "u32", -5, 2, 5), (65, True, "u32", -4, -1, 29),
             (65, False, "u32", -4, -4, 128), (65, False, "u32", -4, -4, 256), (65, False, "u32", -4, -4, 512),
             (65, True, "u32", -4, -4, 512), (65, True, "u32", -4, -3, 1), (65, True, "u32", -4, -2, 1),
             (65, False, "u16", -1, -4, 1), (65, False, "u16", -1, -4, 2), (65, True, "u16", -4, -1, 1), (65, True, "u16", -4, -1, 2),
             (25, False, "u32", -4, -4, 8), (25, False, "u32", -4, -4, 16), (25, True, "u32", -4, -4, 8), (25, True, "u32", -4, -4, 16),
             (17, True, "u32", -4, -4, 2), (17, True, "u32", -4, -4, 4), (13, False, "u32", -4, -4, 1), (13, False, "u32", -4, -4, 2)]


def _edge_name(N, tr, mode, a=0, b=0, t=0):
    return "edge_%d%s_%s" % (N, "t" if tr else "", mode) + ("_%d_%d_%d" % (a, b, t) if t else "")


# ---- b. the centre ------------------------------------------------------------------------------------------------------------------------
def centre_case(N, mode, t):
    """The N x N square (N odd), point-symmetric, the centre pixel brightest; the pixel right of the centre raised by t: the centroid moves
    t / m00 off the centre pixel."""
    c = N // 2
    x, y = np.meshgrid(np.arange(N), np.arange(N))
    x, y = x.ravel(), y.ravel()
    dx, dy = x - c, y - c
    flip = (dx < 0) | ((dx == 0) & (dy < 0))
    key = np.where(flip, -dx, dx) * 1024 + np.where(flip, -dy, dy) + 512
    lo, span, top = _MODE[mode]
    v = lo + _mix(key, 100 + N) % span
    v[(dx == 0) & (dy == 0)] = top
    v[(dx == 1) & (dy == 0)] += t
    return _roi(x, y, v)


def centre_r(roi):
    """r of the centre pixel and whether it is kept."""
    w, _ = box(roi)
    c = w // 2
    k = int(np.flatnonzero((roi["x"] == c) & (roi["y"] == c))[0])
    mem = members(roi)
    return float(mem["r"][k]), bool(mem["keep"][k])


# t of the 13 x 13 32-bit family that puts r of the centre pixel on either side of 1e-12 (m00 = 5.4e11: r = t / (13 m00)), and the
# 93 x 93 32-bit family's first member (m00 = 2^44.7: the smallest positive r any case here reaches)
CENTRE = {"centre_on_pixel_u16": (13, "u16", 0), "centre_on_pixel_u32": (13, "u32", 0), "centre_smallest_r": (93, "u32", 1),
          "centre_r_below_1e-12": (13, "u32", 7), "centre_r_above_1e-12": (13, "u32", 8),
          "centre_r_fast_path": (13, "u32", 4096)}


# ---- c. aspect ----------------------------------------------------------------------------------------------------------------------------
def _line(k, salt):
    return 1 + _mix(np.arange(k), salt) % 250


def strip(w, h, salt):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return _roi(x.ravel(), y.ravel(), _line(w * h, salt))


def empty_disc():
    """Two blobs in a 12 x 1 row, N = 1, the centroid in the gap: every |x| >= 3.5, no pixel in the disc."""
    return _roi([0, 1, 2, 9, 10, 11], [0] * 6, [5, 9, 7, 7, 9, 5])


def l_shape():
    pts = [(i, j) for i in range(21) for j in range(17) if i < 5 or j >= 13]
    x, y = np.array(pts).T
    return _roi(x, y, 1 + _mix(x * 64 + y, 7) % 4000)


def ring_cloud():
    pts = [(i, j) for i in range(31) for j in range(31) if 9 ** 2 <= (i - 15) ** 2 + (j - 15) ** 2 <= 15 ** 2]
    x, y = np.array(pts).T
    return _roi(x, y, 1 + _mix(x * 64 + y, 8) % 60000)


# ---- d. sizes -----------------------------------------------------------------------------------------------------------------------------
SIZES = (2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 4099)


def ragged(npx, W, salt):
    """npx pixels in rows of uneven lengths (W / 2 .. W, the first row full), intensities 0 .. 255 with one in eight zero."""
    xs, ys, j = [], [], 0
    while len(xs) < npx:
        n = W if j == 0 else W - int(_mix([j], salt)[0]) % (W // 2 + 1)
        s = (W - n) // 2 if j % 2 else 0
        take = min(n, npx - len(xs))
        xs += list(range(s, s + take))
        ys += [j] * take
        j += 1
    x, y = np.array(xs), np.array(ys)
    if npx < W:
        x = x - x.min()
    h = _mix(np.arange(npx), salt + 1)
    v = np.where(h % 8 == 0, 0, 1 + (h >> 3) % 255)
    v[0], v[-1] = 255, 3                                                     # never flat
    return _roi(x, y, v)


def _size_width(npx):
    return 16 if npx <= 256 else 40 if npx <= 1025 else 80                   # class 0 (sides <= 32) | class 1 (<= 64) | class 2 (<= 128)


# ---- e. coefficients ----------------------------------------------------------------------------------------------------------------------
def ring_half(N=41):
    """A one-pixel ring of radius N / 2 in the N x N box, intensities uneven (every angular order present)."""
    c = N // 2
    pts = [(i, j) for i in range(N) for j in range(N) if abs(np.hypot(i - c, j - c) - (N // 2)) < 0.5]
    x, y = np.array(pts).T
    v = 1 + _mix(x * 64 + y, 9) % 1000
    v[(x > c) & (abs(y - c) < 4)] += 20000                                   # a bright arc
    return _roi(x, y, v)


def arcs_wide(N=41):
    """Two opposite arcs of radius 0.95 N in the (2N + 1) x N box (the disc is wider than the box's short side), one much brighter."""
    w, h = 2 * N + 1, N
    cx, cy = N, N // 2
    R = 0.95 * N
    pts = [(i, j) for i in range(w) for j in range(h) if abs(np.hypot(i - cx, j - cy) - R) < 0.5]
    pts += [(0, 0), (w - 1, h - 1)]                                          # the box
    x, y = np.array(pts).T
    v = 1 + _mix(x * 64 + y, 10) % 50
    v[(x > cx) & (y > cy)] += 3000
    v[(x < cx)] += 1500
    v[-2:] = 1
    return _roi(x, y, v)


def dumbbell(N=33):
    """Two pixels at opposite corners of the N x N box, weights 3 : 2 -- r = 0.4 sqrt(2) (N - 1) / N and 0.6 sqrt(2) (N - 1) / N."""
    return _roi([0, N - 1], [0, N - 1], [3000, 2000])


def dumbbell_skew():
    return _roi([0, 40], [0, 22], [1000, 3000])


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
def _catalogue():
    cat, groups = {}, {g: [] for g in ("edge", "centre", "aspect", "sizes", "coeff", "aux")}

    def add(group, name, fn, *args):
        assert name not in cat
        cat[name] = functools.partial(fn, *args)
        groups[group].append(name)
    for N in EDGE_N:
        for tr in (False, True):
            for mode in MODES:
                add("edge", _edge_name(N, tr, mode), edge_case, N, tr, mode)
    for k in EDGE_KEPT:
        add("edge", _edge_name(*k), edge_case, *k)
    for name, (N, mode, t) in CENTRE.items():
        add("centre", name, centre_case, N, mode, t)
    for k in (2, 3, 64, 257):
        add("aspect", "row_1x%d" % k, strip, k, 1, k)
        add("aspect", "col_%dx1" % k, strip, 1, k, k + 1)
    add("aspect", "strip_2x65", strip, 65, 2, 20)
    add("aspect", "strip_65x2", strip, 2, 65, 21)
    add("aspect", "empty_disc", empty_disc)
    add("aspect", "l_shape", l_shape)
    add("aspect", "ring_cloud", ring_cloud)
    for n in SIZES:
        add("sizes", "ragged_%d" % n, ragged, n, _size_width(n), n)
    add("sizes", "thin_33", ragged, 80, 33, 33)                              # <= 256 pixels but a side beyond 32: class 1, four waves
    add("aux", "companion_5000", ragged, 5000, 80, 5000)
    add("aux", "companion_40x40", strip, 40, 40, 40)
    add("coeff", "ring_half", ring_half)
    add("coeff", "arcs_wide", arcs_wide)
    add("coeff", "dumbbell", dumbbell)
    add("coeff", "dumbbell_skew", dumbbell_skew)
    return cat, groups


CASES, GROUPS = _catalogue()
CAP_TRIO = ("ragged_4095", "ragged_4096", "ragged_4097")
CLASS0 = "ragged_255"
_CACHE = {}


def roi(name):
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
    return _CACHE[name]


def edge_key(name):
    """(N, transposed) of an edge case."""
    tag = name.split("_")[1]
    return int(tag.rstrip("t")), tag.endswith("t")


def batch(names):
    return _abi.batch_from_rois([roi(n) for n in names])


def golden():
    """{name: {"hash", "npx", "kept", "exact": float64[30]}}"""
    with open(GOLDEN) as f:
        raw = json.load(f)["cases"]
    return {k: {"hash": g["hash"], "npx": g["npx"], "kept": g["kept"], "exact": np.array([float.fromhex(h) for h in g["exact"]])}
            for k, g in raw.items()}
