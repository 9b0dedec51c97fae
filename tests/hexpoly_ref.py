"""numpy-float64 restatement of the reference's HexagonalityPolygonalityFeature (POLYGONALITY_AVE, HEXAGONALITY_AVE,
HEXAGONALITY_STDDEV): own code, written from /root/reference/src/nyx/features/hexagonality_polygonality.cpp:14-165 (calculate) and
:182-217 (the gates of parallel_process_1_batch), in the reference's operation order.  Every operation is a numpy float64 +, -, *, /
or square root (IEEE, unfused; a division by zero gives the infinity it gives in C++), and the one tangent is math.tan: the libm the
reference calls.  tests/test_hexpoly_cpu.py pins `closing` to values recorded from the reference's class (tests/golden/hexpoly), bit
for bit; `table` then serves arbitrary batches (the GPU tests, tools/hexpoly_fuzz.py) on top of neighbors_ref, morph_ref and
caliper_ref, each of which is pinned to the reference in the same way."""
from __future__ import annotations

import math

import numpy as np

NAMES = ["POLYGONALITY_AVE", "HEXAGONALITY_AVE", "HEXAGONALITY_STDDEV"]
INPUTS = ["N_PIXELS", "N_CONTOUR", "NUM_NEIGHBORS", "PERIMETER", "CONVEX_HULL_AREA", "STAT_FERET_DIAM_MIN", "STAT_FERET_DIAM_MAX"]
NOVALUE = -1.0               # HexagonalityPolygonalityFeature::novalue
TAN_TABLE_CAP = 128          # kHexpolyTanCap: up to this neighbor count the HIP path takes tan(M_PI / k) from the host's libm

F = np.float64


def _ratio_stats(vals, skip_nonfinite):
    """(mean, population deviation) of 1 - |1 - a / b| over ib < ic in loop order, summed one after the other (:84-104, :132-147)."""
    kept = []
    s = F(0.0)
    for ib in range(len(vals)):
        for ic in range(ib + 1, len(vals)):
            r = F(1.0) - abs(F(1.0) - vals[ib] / vals[ic])
            if skip_nonfinite and not np.isfinite(r):
                continue
            kept.append(r)
            s = s + r
    n = F(len(kept))
    ave = s / n
    sq = F(0.0)
    for r in kept:
        sq = sq + (r - ave) * (r - ave)
    return ave, np.sqrt(sq / n)


def closing(n_px, n_contour, neighbors, perimeter, hull_area, feret_min, feret_max):
    """The three columns of one ROI from its six numbers and its contour length."""
    with np.errstate(all="ignore"):
        nbd = F(neighbors)
        area_hull = F(hull_area)
        # parallel_process_1_batch:202 -- no contour, CONVEX_HULL_AREA == 0, NUM_NEIGHBORS == 0
        if int(n_contour) == 0 or area_hull == 0 or nbd == 0:
            return [NOVALUE] * 3
        nb = int(nbd)                                    # size_t neighbors = fvals[NUM_NEIGHBORS][0]
        if nb < 3:                                       # :49, :159
            return [NOVALUE] * 3
        neighbors = F(nb)
        area = F(int(n_px))                              # aux_area
        perimeter, min_feret, max_feret = F(perimeter), F(feret_min), F(feret_max)
        s3 = np.sqrt(F(3.0))
        perim_hull = F(6.0) * np.sqrt(area_hull / (F(1.5) * s3))
        perimeter_neighbors = perimeter / neighbors
        t = F(math.tan(math.pi / float(nb)))
        poly_size_ratio = F(1.0) - abs(F(1.0) - perimeter_neighbors / np.sqrt((F(4.0) * area) / (neighbors / t)))
        poly_area_ratio = F(1.0) - abs(F(1.0) - area / (F(0.25) * neighbors * perimeter_neighbors * perimeter_neighbors / t))
        poly_ave = F(10.0) * (poly_size_ratio + poly_area_ratio) / F(2.0)
        apoth1, apoth2, apoth3 = s3 * perimeter / F(12.0), s3 * max_feret / F(4.0), min_feret / F(2.0)
        side1, side2, side3, side4 = perimeter / F(6.0), max_feret / F(2.0), min_feret / s3, perim_hull / F(6.0)
        hexc = F(0.5) * (F(3.0) * s3)
        list_area = [hexc * side1 * side1, hexc * side2 * side2, hexc * side3 * side3, F(3.0) * side1 * apoth2, F(3.0) * side1 * apoth3,
                     F(3.0) * side2 * apoth3, F(3.0) * side4 * apoth1, F(3.0) * side4 * apoth2, F(3.0) * side4 * apoth3, area_hull, area]
        area_ave, area_sd = _ratio_stats(list_area, True)
        apoth4 = s3 * perim_hull / F(12.0)
        apoth5 = np.sqrt(F(4.0) * area_hull / (F(4.5) * s3))
        list_perim = [np.sqrt(F(24.0) * area / s3), np.sqrt(F(24.0) * area_hull / s3), perimeter, perim_hull, F(3.0) * max_feret,
                      F(6.0) * min_feret / s3, F(2.0) * area / apoth1, F(2.0) * area / apoth2, F(2.0) * area / apoth3, F(2.0) * area / apoth4,
                      F(2.0) * area / apoth5, F(2.0) * area_hull / apoth1, F(2.0) * area_hull / apoth2, F(2.0) * area_hull / apoth3]
        perim_ave, perim_sd = _ratio_stats(list_perim, False)
        hex_sd = np.sqrt((area_sd * area_sd + perim_sd * perim_sd) / F(2.0))
        hex_ave = F(10.0) * (area_ave + perim_ave) / F(2.0)
        return [float(poly_ave), float(hex_ave), float(hex_sd)]


def closing_rows(inputs):
    """(n, 3) from (n, 7) rows of INPUTS."""
    return np.array([closing(*row) for row in np.asarray(inputs, np.float64)], np.float64).reshape(len(inputs), 3)


def inputs_of(b, distance, contours=None):
    """(n_roi, 7): INPUTS of every ROI of a HostBatch, from the restatements of the classes that produce them."""
    from tests import caliper_ref, morph_ref, neighbors_ref
    if contours is None:
        from tests.radial_ref import contours_of
        contours = contours_of(b)
    nb = neighbors_ref.table(b, distance, contours)
    mo = morph_ref.table(b, contours)
    ca = caliper_ref.table(b)
    m, c = morph_ref.NAMES.index, caliper_ref.NAMES.index
    n_px = np.diff(np.asarray(b.px_offset).astype(np.int64)).astype(np.float64)
    return np.column_stack([n_px, nb[:, 9], nb[:, 0], mo[:, m("PERIMETER")], mo[:, m("CONVEX_HULL_AREA")], ca[:, c("STAT_FERET_DIAM_MIN")],
                            ca[:, c("STAT_FERET_DIAM_MAX")]])


def table(b, distance, contours=None):
    """(n_roi, 3): the columns of NAMES, raw (-1 where a gate closes; NaN / inf where the reference has them)."""
    return closing_rows(inputs_of(b, distance, contours))


def same_bits(a, b):
    """Equal as bit patterns, any NaN matching any NaN (a NaN's payload and sign are not part of the reference's contract)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool((((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))).all())
