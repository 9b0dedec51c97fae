"""numpy / Python-int restatement of four classes of the reference's shape block, as the HIP path serves them
(nyxus_amd/csrc/roi_morph.hip):

    BasicMorphologyFeatures  features/basic_morphology.cpp:19-92
    ContourFeature           features/contour.cpp:935-1021 (the merged contour: tests/radial_ref.contours_of)
    ConvexHullFeature        features/convex_hull_nontriv.cpp:18-33, :53-120, :193-213
    ExtremaFeature           features/extrema.cpp:15-74

Takes a HostBatch plus the ROIs' merged contours (padded coordinates, walk order).  Integer sums are Python integers, converted
once and divided once; PERIMETER adds its terms one after the other.  Three columns are formed by the reference with an on-line
(Welford) update whose roundings depend on the order -- COMPACTNESS, EDGE_MEAN_INTENSITY, EDGE_STDDEV_INTENSITY: here they are the
EXACT rational mean and centred sum of squares of the same fp64 terms, rounded once, so that a tolerance against this module is not
spent on the restatement's own rounding.  tests/test_morph_cpu.py pins this module to values recorded from the classes."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from tests import circle_ref  # noqa: F401  (the perimeter's order is restated there as well)

BASIC = ["AREA_PIXELS_COUNT", "AREA_UM2", "CENTROID_X", "CENTROID_Y", "WEIGHTED_CENTROID_Y", "WEIGHTED_CENTROID_X", "MASS_DISPLACEMENT",
         "COMPACTNESS", "BBOX_YMIN", "BBOX_XMIN", "BBOX_HEIGHT", "BBOX_WIDTH", "DIAMETER_EQUAL_AREA", "EXTENT", "ASPECT_RATIO"]
CONTOUR = ["PERIMETER", "DIAMETER_EQUAL_PERIMETER", "EDGE_MEAN_INTENSITY", "EDGE_STDDEV_INTENSITY", "EDGE_MAX_INTENSITY", "EDGE_MIN_INTENSITY",
           "EDGE_INTEGRATED_INTENSITY"]
HULL = ["CIRCULARITY", "CONVEX_HULL_AREA", "SOLIDITY"]
EXTREMA = ["EXTREMA_P%d_%s" % (k, a) for k in range(1, 9) for a in "XY"]
NAMES = BASIC + CONTOUR + HULL + EXTREMA
ROUNDED = ["COMPACTNESS", "EDGE_MEAN_INTENSITY", "EDGE_STDDEV_INTENSITY"]      # agree with the reference to rounding; every other column bit for bit
POSITION = ["CENTROID_X", "CENTROID_Y", "WEIGHTED_CENTROID_X", "WEIGHTED_CENTROID_Y", "BBOX_XMIN", "BBOX_YMIN"] + EXTREMA
# Formed from the ROUNDED absolute centroids (the reference's order of operations), so their last bits move with the origin.  Each
# centroid carries half an ulp of the coordinate; a difference of two and a square root of two squares at most doubles that twice:
# 8 ulp of the largest coordinate bounds the change between two placements (COMPACTNESS is divided by n >= 1 besides).
CENTROID_BOUND = ["MASS_DISPLACEMENT", "COMPACTNESS"]
CENTROID_ULPS = 8
POSITION_X =[n for n in POSITION if n.endswith("X") or n.endswith("XMIN")]
BITS = {"BASIC": 1, "CONTOUR": 2, "HULL": 4, "EXTREMA": 8}
BLOCKS = {1: BASIC, 2: CONTOUR, 4: HULL, 8: EXTREMA}


def names_of(mask):
    return [n for bit in (1, 2, 4, 8) if mask & bit for n in BLOCKS[bit]]


def columns_of(mask):
    """Indices into the 41 columns of the full table of the columns of `mask`, in order."""
    return [NAMES.index(n) for n in names_of(mask)]


def _exact_mean_m2(vals):
    """(mean, centred sum of squares) of doubles or integers as exact rationals."""
    fr = [Fraction(v) for v in vals]
    n = len(fr)
    s = sum(fr)
    s2 = sum(f * f for f in fr)
    return s / n, s2 - s * s / n


def _right_turn(p1, p2, p3):
    return (p3[0] - p1[0]) * (p2[1] - p1[1]) - (p3[1] - p1[1]) * (p2[0] - p1[0]) > 0


def convex_hull(pts):
    """ConvexHullFeature::build_convex_hull over a list of (x, y) Python-int pairs: the reference's vertex order."""
    if len(pts) < 2:
        return []
    o = sorted(pts)
    n = len(o)
    up = [o[0], o[1]]
    for i in range(2, n):
        while len(up) > 1 and not _right_turn(up[-2], up[-1], o[i]):
            up.pop()
        up.append(o[i])
    lo = [o[n - 1], o[n - 2]]
    for i in range(2, n):
        while len(lo) > 1 and not _right_turn(lo[-2], lo[-1], o[n - i - 1]):
            lo.pop()
        lo.append(o[n - i - 1])
    seen = set(up)
    for p in lo:
        if p not in seen:
            up.append(p)
            seen.add(p)
    return up


def hull_area(h):
    """polygon_area + hull_boundary_points / 2 + 1 (convex_hull_nontriv.cpp:60): sums of halves, exact."""
    a2, b = 0, 0
    n = len(h)
    for i in range(n):
        p, q = h[i], h[(i + 1) % n]
        a2 += p[0] * q[1] - p[1] * q[0]
        if n >= 2:
            b += math.gcd(abs(q[0] - p[0]), abs(q[1] - p[1]))
    return abs(a2) / 2.0 + b / 2.0 + 1.0


def roi_row(x, y, v, K, ox, oy, w, h):
    """The 41 columns of one ROI: x, y box-relative cloud, v intensities, K (nK, 2) padded contour, (ox, oy) the box origin."""
    n = len(x)
    row = np.zeros(len(NAMES))
    if n == 0:
        return row
    X = [int(a) + int(ox) for a in x]
    Y = [int(a) + int(oy) for a in y]
    V = [int(a) for a in v]
    c = {k: i for i, k in enumerate(NAMES)}
    # ---- basic morphology
    cx, cy = float(sum(X)) / float(n), float(sum(Y)) / float(n)
    dx, dy = np.asarray(X, np.float64) - cx, np.asarray(Y, np.float64) - cy
    d = np.sqrt(dx * dx + dy * dy)
    _, m2 = _exact_mean_m2(d.tolist())
    std = math.sqrt(float(m2 / (n - 1))) if n > 2 else 0.0
    mass = sum(V)
    if mass > 0:
        wcx, wcy = float(sum(a * b for a, b in zip(X, V))) / float(mass), float(sum(a * b for a, b in zip(Y, V))) / float(mass)
    else:
        wcx = wcy = 0.0
    ddx, ddy = wcx - cx, wcy - cy
    row[c["AREA_PIXELS_COUNT"]] = n
    row[c["AREA_UM2"]] = 0.0
    row[c["CENTROID_X"]], row[c["CENTROID_Y"]] = cx, cy
    row[c["WEIGHTED_CENTROID_X"]], row[c["WEIGHTED_CENTROID_Y"]] = wcx, wcy
    row[c["MASS_DISPLACEMENT"]] = math.sqrt(ddx * ddx + ddy * ddy)
    row[c["COMPACTNESS"]] = std / float(n)
    row[c["BBOX_YMIN"]], row[c["BBOX_XMIN"]], row[c["BBOX_HEIGHT"]], row[c["BBOX_WIDTH"]] = oy, ox, h, w
    row[c["DIAMETER_EQUAL_AREA"]] = 2.0 * math.sqrt(float(n) / math.pi)
    row[c["EXTENT"]] = float(n) / float(int(w) * int(h))
    row[c["ASPECT_RATIO"]] = float(w) / float(h)
    # ---- contour
    nK = len(K)
    per = 0.0
    if nK:
        KX, KY = np.asarray(K[:, 0], np.int64), np.asarray(K[:, 1], np.int64)
        ex, ey = KX - np.roll(KX, 1), KY - np.roll(KY, 1)                    # term 0: the last point to the first
        for t in np.sqrt((ex * ex + ey * ey).astype(np.float64)):
            per += float(t)                                                  # the reference's order
        plane = {(int(a), int(b)): val for a, b, val in zip(x, y, V)}
        I = [plane[(int(a) - 1, int(b) - 1)] for a, b in zip(KX, KY)]       # padded coordinates: the pixel is (kx - 1, ky - 1)
        em, em2 = _exact_mean_m2(I)
        row[c["PERIMETER"]] = per
        row[c["DIAMETER_EQUAL_PERIMETER"]] = per / math.pi
        row[c["EDGE_MEAN_INTENSITY"]] = float(em)
        row[c["EDGE_STDDEV_INTENSITY"]] = math.sqrt(float(em2 / (nK - 1))) if nK > 2 else 0.0
        row[c["EDGE_MAX_INTENSITY"]], row[c["EDGE_MIN_INTENSITY"]] = max(I), min(I)
        row[c["EDGE_INTEGRATED_INTENSITY"]] = float(sum(I))
    # ---- convex hull
    area = hull_area(convex_hull(list(zip(X, Y))))
    with np.errstate(divide="ignore"):
        row[c["CIRCULARITY"]] = np.sqrt(np.float64(4.0 * math.pi * float(n)) / np.float64(per * per))
    row[c["CONVEX_HULL_AREA"]] = area
    row[c["SOLIDITY"]] = float(n) / area
    # ---- extrema (tight boxes: the top row is y = oy, ...)
    top, bot, lef, rig = min(Y), max(Y), min(X), max(X)
    P = [(min(a for a, b in zip(X, Y) if b == top), top), (max(a for a, b in zip(X, Y) if b == top), top),
         (rig, min(b for a, b in zip(X, Y) if a == rig)), (rig, max(b for a, b in zip(X, Y) if a == rig)),
         (max(a for a, b in zip(X, Y) if b == bot), bot), (min(a for a, b in zip(X, Y) if b == bot), bot),
         (lef, max(b for a, b in zip(X, Y) if a == lef)), (lef, min(b for a, b in zip(X, Y) if a == lef))]
    for k, (px, py) in enumerate(P):
        row[c["EXTREMA_P%d_X" % (k + 1)]], row[c["EXTREMA_P%d_Y" % (k + 1)]] = px, py
    return row


def table(b, contours=None):
    """(n_roi, 41): the columns of NAMES (raw: CIRCULARITY is +inf without a contour)."""
    if contours is None:
        from tests.radial_ref import contours_of
        contours = contours_of(b)
    T = np.zeros((b.n_roi, len(NAMES)))
    for r in range(b.n_roi):
        o, e = int(b.px_offset[r]), int(b.px_offset[r + 1])
        ox = int(b.origin_x[r]) if b.origin_x is not None else 0
        oy = int(b.origin_y[r]) if b.origin_y is not None else 0
        T[r] = roi_row(b.x[o:e], b.y[o:e], b.inten[o:e], contours[r], ox, oy, int(b.bbox_w[r]), int(b.bbox_h[r]))
    return T
