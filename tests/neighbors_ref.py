"""Brute-force restatement of the reference's NeighborsFeature (NUM_NEIGHBORS, PERCENT_TOUCHING, CLOSEST_NEIGHBOR{1,2}_{DIST,ANG},
ANG_BW_NEIGHBORS_{MEAN,STDDEV,MODE}): own code, written from /root/reference/src/nyx/features/neighbors.cpp:21-27, :125-536 (the
single-thread branch), features/pixel.cpp:75-88 (exact_min_sqdist), features/moments.h:15-38 (Moments2) and
features/basic_morphology.cpp:40-47 (the centroid).

Takes a HostBatch whose rows ascend in label inside every image (HostBatch.image_offset; None: one image) with the boxes' origins, plus
the ROIs' merged contours (tests/radial_ref.contours_of: padded box coordinates -- the padding is the same for every ROI, so it drops out
of every difference).  Angles, roots and the Welford recurrence are written with math.atan2, math.sqrt and plain float arithmetic,
literally as the reference has them, so that the restatement shares the reference's libm.  tests/test_neighbors_cpu.py pins this module
to values recorded from the reference's class (tests/golden/neighbors); it then serves arbitrary inputs (tools/neighbors_fuzz.py).
"""
from __future__ import annotations

import math

import numpy as np

NAMES = ["NUM_NEIGHBORS", "PERCENT_TOUCHING", "CLOSEST_NEIGHBOR1_DIST", "CLOSEST_NEIGHBOR1_ANG", "CLOSEST_NEIGHBOR2_DIST",
         "CLOSEST_NEIGHBOR2_ANG", "ANG_BW_NEIGHBORS_MEAN", "ANG_BW_NEIGHBORS_STDDEV", "ANG_BW_NEIGHBORS_MODE"]
EXTRA = ["N_CONTOUR", "CENTROID_X", "CENTROID_Y"]
EXACT = {"NUM_NEIGHBORS", "PERCENT_TOUCHING", "CLOSEST_NEIGHBOR1_DIST", "CLOSEST_NEIGHBOR2_DIST", "ANG_BW_NEIGHBORS_MODE"}
TOUCH2 = 2                   # touchThresh2, neighbors.cpp:243


def direction_angle_deg(x1, y1, x2, y2):
    ang = math.atan2(y2 - y1, x2 - x1) * 180.0 / math.pi
    if ang < 0.0:
        ang += 360.0
    return ang


def image_ranges(b):
    io = b.image_offset
    if io is None:
        return [(0, b.n_roi)]
    return [(int(io[k]), int(io[k + 1])) for k in range(len(io) - 1)]


def centroids(b):
    """CENTROID_X / _Y: sums of absolute coordinates (exact integers) divided by the pixel count."""
    off = np.asarray(b.px_offset).astype(np.int64)
    out = np.zeros((b.n_roi, 2))
    for r in range(b.n_roi):
        o, n = int(off[r]), int(off[r + 1] - off[r])
        ox = int(b.origin_x[r]) if b.origin_x is not None else 0
        oy = int(b.origin_y[r]) if b.origin_y is not None else 0
        sx = int(np.asarray(b.x[o:o + n], np.int64).sum()) + n * ox
        sy = int(np.asarray(b.y[o:o + n], np.int64).sum()) + n * oy
        out[r] = (float(sx) / float(n), float(sy) / float(n))
    return out


def table(b, radius, contours=None, with_stats=False):
    """(n_roi, 12): the nine columns, then the contour length and the centroid.  with_stats: also a dict of what the run met
    (candidate pairs, pairs skipped for an empty contour, contour points near several neighbors, the largest candidate list)."""
    if contours is None:
        from tests.radial_ref import contours_of
        contours = contours_of(b)
    R = int(radius)
    n = b.n_roi
    ox = np.asarray(b.origin_x, np.int64) if b.origin_x is not None else np.zeros(n, np.int64)
    oy = np.asarray(b.origin_y, np.int64) if b.origin_y is not None else np.zeros(n, np.int64)
    xmin, ymin = ox, oy
    xmax, ymax = ox + np.asarray(b.bbox_w, np.int64) - 1, oy + np.asarray(b.bbox_h, np.int64) - 1
    K = [np.asarray(k, np.int64).reshape(-1, 2) + np.array([ox[r], oy[r]], np.int64) for r, k in enumerate(contours)]
    cen = centroids(b)
    T = np.zeros((n, 12))
    T[:, 9] = [len(k) for k in K]
    T[:, 10:] = cen
    stats = {"candidates": 0, "skipped_empty": 0, "multi_touch_points": 0, "max_candidates": 0, "touch_not_neighbor": 0}
    labels = np.asarray(b.roi_label, np.int64)
    for lo, hi in image_ranges(b):
        assert (np.diff(labels[lo:hi]) > 0).all(), "rows of an image must ascend strictly in label"
        touch = {r: np.zeros(len(K[r]), np.int64) for r in range(lo, hi)}      # per contour INDEX: how many neighbors lie within TOUCH2
        neigh = {r: [] for r in range(lo, hi)}
        n_cand = np.zeros(hi - lo, np.int64)
        for a in range(lo, hi):
            no = ((xmin[a + 1:hi] - R > xmax[a] + R) | (xmax[a + 1:hi] + R < xmin[a] - R)
                  | (ymin[a + 1:hi] - R > ymax[a] + R) | (ymax[a + 1:hi] + R < ymin[a] - R))       # aabbNoOverlap
            for b_ in (np.nonzero(~no)[0] + a + 1):
                b_ = int(b_)
                stats["candidates"] += 1
                if len(K[a]) == 0 or len(K[b_]) == 0:
                    stats["skipped_empty"] += 1
                    continue
                n_cand[a - lo] += 1
                n_cand[b_ - lo] += 1
                d = K[a][:, None, :] - K[b_][None, :, :]
                D = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
                da, db = D.min(axis=1), D.min(axis=0)
                touch[a] += da <= TOUCH2                                       # BEFORE the radius gate
                touch[b_] += db <= TOUCH2
                mind = int(da.min())
                if mind > R * R:
                    if mind <= TOUCH2:
                        stats["touch_not_neighbor"] += 1
                    continue
                neigh[a].append(b_)
                neigh[b_].append(a)
        stats["max_candidates"] = max(stats["max_candidates"], int(n_cand.max()) if len(n_cand) else 0)
        for r in range(lo, hi):
            nb = neigh[r]                                                      # ascending: the processing order of the pairs
            assert nb == sorted(nb)
            T[r, 0] = float(len(nb))
            nt = int((touch[r] > 0).sum())
            stats["multi_touch_points"] += int((touch[r] > 1).sum())
            T[r, 1] = 100.0 * float(nt) / float(len(K[r])) if len(K[r]) else 0.0
            if not nb:
                continue
            cx, cy = float(cen[r, 0]), float(cen[r, 1])
            dists = []
            for q in nb:
                dx, dy = cx - float(cen[q, 0]), cy - float(cen[q, 1])
                dists.append(math.sqrt(dx * dx + dy * dy))
            i1 = dists.index(min(dists))                                       # std::min_element: the first minimum
            T[r, 2] = dists[i1]
            T[r, 3] = direction_angle_deg(cx, cy, float(cen[nb[i1], 0]), float(cen[nb[i1], 1]))
            if len(nb) > 1:
                rest = list(dists)
                rest[i1] = math.inf
                i2 = rest.index(min(rest))
                T[r, 4] = dists[i2]
                T[r, 5] = direction_angle_deg(cx, cy, float(cen[nb[i2], 0]), float(cen[nb[i2], 1]))
            mean, m2, cnt = 0.0, 0.0, 0                                        # Moments2::add
            counts = [0] * 361
            for q in nb:
                ang = direction_angle_deg(cx, cy, float(cen[q, 0]), float(cen[q, 1]))
                n1 = cnt
                cnt = cnt + 1
                delta = ang - mean
                delta_n = delta / float(cnt)
                term1 = delta * delta_n * float(n1)
                mean = mean + delta_n
                m2 += term1
                ra = int(math.floor(ang + 0.5)) if ang >= 0 else -int(math.floor(-ang + 0.5))      # std::round: halves away from zero
                counts[max(0, min(360, ra))] += 1
            T[r, 6] = mean
            T[r, 7] = math.sqrt(m2 / float(cnt - 1)) if cnt > 2 else 0.0
            T[r, 8] = float(counts.index(max(counts)))                         # the smallest angle among those with the highest count
    return (T, stats) if with_stats else T
