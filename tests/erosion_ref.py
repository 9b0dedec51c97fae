"""numpy restatement of two classes of the reference's shape block, as the HIP path serves them (nyxus_amd/csrc/roi_erosion.hip):

    ErosionPixelsFeature   features/erosion.cpp:20-109 and the aux_min == aux_max skip of its driver (:147-164)
    EllipseFittingFeature  features/ellipse_fitting.cpp:26-82 (centroid and area: basic_morphology.cpp:21-47)

The erosion value is an integer and equals the reference bit for bit.  The ellipse columns are formed from exact integer sums of the
box-relative coordinates, with the device's operations in the device's order (Python floats are IEEE doubles and never fused), so
they differ from the reference -- fp64 sums about a rounded centroid -- by rounding only.  exact() gives the moments as Fractions:
the generator and the CPU test derive from them which ORIENTATION / ECCENTRICITY values are compared."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

ELLIPSE = ["MAJOR_AXIS_LENGTH", "MINOR_AXIS_LENGTH", "ELONGATION", "ECCENTRICITY", "ORIENTATION", "ROUNDNESS"]
EROSION = ["EROSIONS_2_VANISH", "EROSIONS_2_VANISH_COMPLEMENT"]
NAMES = ELLIPSE + EROSION
MAX_PASSES = 1000                    # SANITY_MAX_NUM_EROSIONS
NOISE = 1e-6                         # bound of the `compared` mask, relative to uxx + uyy


def erosions_to_vanish(x, y, w, h, min_inten, max_inten):
    if len(x) == 0 or int(min_inten) == int(max_inten):
        return 0                                                             # skipped by the driver: the initial value
    w, h = int(w), int(h)
    cur = np.zeros((h, w), bool)
    cur[np.asarray(y, np.int64), np.asarray(x, np.int64)] = True             # whatever the intensity
    if w < 4 or h < 4:
        return 0                                                             # empty loops: numNon0 == 0 at the first pass
    for k in range(MAX_PASSES):
        # columns 2 <= c < w - 1, rows 2 <= r < h - 1: the cell AND its four edge neighbours; every other cell is copied
        sub = cur[2:h - 1, 2:w - 1] & cur[1:h - 2, 2:w - 1] & cur[3:h, 2:w - 1] & cur[2:h - 1, 1:w - 2] & cur[2:h - 1, 3:w]
        if not sub.any():
            return k
        if (sub == cur[2:h - 1, 2:w - 1]).all():
            return MAX_PASSES                                                # nothing changed and something is left: every later pass is this one
        cur = cur.copy()
        cur[2:h - 1, 2:w - 1] = sub
    return MAX_PASSES


def sums(x, y):
    """n, sum x, sum y, sum x^2, sum y^2, sum xy as Python integers."""
    xs, ys = [int(v) for v in x], [int(v) for v in y]
    return (len(xs), sum(xs), sum(ys), sum(v * v for v in xs), sum(v * v for v in ys), sum(a * b for a, b in zip(xs, ys)))


def _to_double(v):
    """The device's rounding of a 128-bit value: the high word times 2^64 plus the low word."""
    return float(v >> 64) * 18446744073709551616.0 + float(v & 0xFFFFFFFFFFFFFFFF)


def ellipse(x, y):
    n, sx, sy, sxx, syy, sxy = sums(x, y)
    if n == 0:
        return [0.0] * 6
    nxx, nyy, nxy = n * sxx - sx * sx, n * syy - sy * sy, n * sxy - sx * sy
    nn = float(n) * float(n)
    uxx = _to_double(nxx) / nn + 1. / 12.
    uyy = _to_double(nyy) / nn + 1. / 12.
    uxy = _to_double(abs(nxy)) / nn
    if nxy < 0:
        uxy = -uxy
    common = math.sqrt((uxx - uyy) * (uxx - uyy) + 4. * uxy * uxy)
    major = 2. * math.sqrt(2.) * math.sqrt(uxx + uyy + common)
    minor = 2. * math.sqrt(2.) * math.sqrt(uxx + uyy - common)
    ecc = math.sqrt(1.0 - minor * minor / (major * major))
    elong = minor / major
    rnd = (4. * float(n)) / (math.pi * major * major)
    if uyy > uxx:
        num = uyy - uxx + math.sqrt((uyy - uxx) * (uyy - uxx) + 4 * uxy * uxy)
        den = 2 * uxy
    else:
        num = 2 * uxy
        den = uxx - uyy + math.sqrt((uxx - uyy) * (uxx - uyy) + 4 * uxy * uxy)
    if nxy == 0:
        orient = 0. if uxx >= uyy else 90.
    else:
        orient = 180. / math.pi * math.atan(num / den)
    return [major, minor, elong, ecc, orient, rnd]


def exact(x, y):
    """(uxx, uyy, uxy, common^2) as Fractions."""
    n, sx, sy, sxx, syy, sxy = sums(x, y)
    uxx = Fraction(n * sxx - sx * sx, n * n) + Fraction(1, 12)
    uyy = Fraction(n * syy - sy * sy, n * n) + Fraction(1, 12)
    uxy = Fraction(n * sxy - sx * sy, n * n)
    return uxx, uyy, uxy, (uxx - uyy) ** 2 + 4 * uxy * uxy


def compared(x, y, ref_orientation):
    """Which of the eight columns of this ROI are compared with the reference's values.  For an axis-symmetric shape the reference's
    uxy and `common` are rounding noise about an exact zero: ORIENTATION is compared where |uxy| >= 1e-6 (uxx + uyy), or where uxy is
    exactly 0 and the reference returned exactly 0.0 or 90.0; ECCENTRICITY where common >= 1e-6 (uxx + uyy)."""
    uxx, uyy, uxy, c2 = exact(x, y)
    lim = Fraction(NOISE) * (uxx + uyy)
    m = np.ones(8, bool)
    m[ELLIPSE.index("ORIENTATION")] = abs(uxy) >= lim or (uxy == 0 and float(ref_orientation) in (0.0, 90.0))
    m[ELLIPSE.index("ECCENTRICITY")] = c2 >= lim * lim
    return m


def rois_of(b):
    for r in range(b.n_roi):
        o, e = int(b.px_offset[r]), int(b.px_offset[r + 1])
        yield r, b.x[o:e], b.y[o:e]


def table(b, erosion=True):
    """(n_roi, 8): the ellipse columns, EROSIONS_2_VANISH, EROSIONS_2_VANISH_COMPLEMENT (never assigned by the class: 0)."""
    T = np.zeros((b.n_roi, 8))
    for r, x, y in rois_of(b):
        T[r, :6] = ellipse(x, y)
        if erosion:
            T[r, 6] = erosions_to_vanish(x, y, b.bbox_w[r], b.bbox_h[r], b.min_inten[r], b.max_inten[r])
    return T
