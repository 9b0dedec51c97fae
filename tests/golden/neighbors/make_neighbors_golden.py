#!/usr/bin/env python3
"""Generates tests/golden/neighbors/neighbors_reference.npz, branches.json and api_expected.json: the output of the reference's own
NeighborsFeature::manual_reduce (behind BasicMorphologyFeatures and ContourFeature, its dependencies) on the inputs of
tests/neighbors_cases.py, image by image, at every radius a case names.  Only DATA is stored (per ROI the nine columns, the contour
length and the centroid); the inputs are rebuilt from parameters by tests/neighbors_cases.py.

The reference classes are compiled OUTSIDE the repository: ref_neighbors_driver.cpp (own code, next to this file) against the
reference sources where they lie, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    REF=/root/reference/src/nyx; W=$(mktemp -d)
    for f in features/neighbors features/basic_morphology; do
        g++ -std=c++20 -O2 -fPIC -w -I/opt/conda/include -c $REF/$f.cpp -o $W/$(basename $f).o; done
    g++ -std=c++20 -O2 -fPIC -shared -w -I$REF -Iinclude -I/opt/conda/include -o $W/libnbref.so \\
        tests/golden/neighbors/ref_neighbors_driver.cpp $W/*.o \\
        $(find oracle/_ref/obj -name '*.o') /usr/lib/x86_64-linux-gnu/libtiff.so.5 -lpthread
    NEIGHBORSREF_SO=$W/libnbref.so python tests/golden/neighbors/make_neighbors_golden.py

Every value of every ROI is compared, bit for bit, with tests/neighbors_ref.py before it is stored.  The generator asserts on the
RECORDED data every property the tests rely on (the list in check_branches) and the two conditions that keep the device's atan2 out of
a decision: no recorded angle within 1e-6 of a half-integer unless it is an exact integer (the rounding of ANG_BW_NEIGHBORS_MODE), and
every non-zero ANG_BW_NEIGHBORS_STDDEV at least 1e-3 of its mean.

With NEIGHBORSREF_TIME=1 it also times the reference class (one thread: NeighborsFeature::manual_reduce sets n_threads = 1) on the
inputs of tools/neighbors_probe.py and prints the seconds.

The reference's Python package is not built here, so api_expected.json holds driver-recorded tables with the reference's user-facing
column names (featureset.cpp UserFacingFeatureNames).
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
from tests import neighbors_cases as nc, neighbors_ref as nr  # noqa: E402
from tests.radial_ref import contours_of  # noqa: E402


def load():
    lib = C.CDLL(os.environ["NEIGHBORSREF_SO"])
    lib.neighborsref_batch.restype = C.c_int
    lib.neighborsref_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, radius):
    cb = b.c_struct()
    out = np.zeros((b.n_roi, 12))
    sec = np.zeros(1)
    io = b.image_offset if b.image_offset is not None else np.array([0, b.n_roi], np.uint64)
    rc = lib.neighborsref_batch(C.byref(cb), b.origin_x.ctypes.data, b.origin_y.ctypes.data, io.ctypes.data, len(io) - 1, int(radius),
                                out.ctypes.data, sec.ctypes.data)
    assert rc == 0, rc
    return out, float(sec[0])


def row_of(b, label, image=0):
    lo, hi = nr.image_ranges(b)[image]
    return lo + int(np.nonzero(np.asarray(b.roi_label[lo:hi]) == label)[0][0])


def check_branches(G):
    """The named branches, on the recorded data.  Returns what tests/test_neighbors_cpu.py asserts again from branches.json."""
    C5, C2, C1 = G[("contacts", 5)], G[("contacts", 2)], G[("contacts", 1)]
    b = nc.batch("contacts")
    r = lambda lab: row_of(b, lab)
    assert (C5[r(90), :9] == 0).all() and (C1[r(90), :9] == 0).all()                      # an isolated ROI
    assert C1[r(11), 0] == 1 and C1[r(11), 1] > 0                                         # edge contact: d = 1
    assert C1[r(21), 0] == 0 and C1[r(21), 1] > 0                                         # diagonal only at R = 1: touching, NOT a neighbor
    assert C2[r(21), 0] == 1 and C2[r(21), 1] == C1[r(21), 1]                             # ... a neighbor at R = 2 (d = 2 <= 4)
    assert C1[r(31), 0] == 0 and C2[r(31), 0] == 1 and C2[r(31), 1] == 0                  # a one-pixel gap (d = 4): no touch
    assert C5[r(41), 0] == 1 and C5[r(51), 0] == 0                                        # gap exactly R | gap R + 1 (candidate, not neighbor)
    assert C2[r(61), 0] == 1 and C2[r(71), 0] == 0 and C5[r(71), 0] == 1                  # the same at R = 2
    T = G[("tiny", 5)]
    assert T[:, 9].tolist() == [32, 0, 0, 0] and (T[:, :9] == 0).all()                    # empty contours: the pairs are skipped on both sides
    K2 = G[("corner", 2)]
    assert K2[0, 0] == 2 and K2[1, 0] == 2 and K2[0, 1] <= 100.0
    Ti = G[("ties", 5)]
    bt = nc.batch("ties")
    five = row_of(bt, 5)
    assert Ti[five, 0] == 3 and Ti[five, 2] == Ti[five, 4] == 8.0 and Ti[five, 3] == 180.0 and Ti[five, 5] == 0.0   # the lower labels win
    assert Ti[five, 7] > 0                                                                # >= 3 neighbors: a deviation
    for lab in (20, 21):
        q = row_of(bt, lab)
        assert Ti[q, 0] == 1 and Ti[q, 2] == 0.0 and Ti[q, 3] == 0.0                      # the same centroid: distance 0, angle 0
    R4 = G[("row4", 12)]
    assert R4[0, 0] == 3 and R4[0, 6] == 0.0 and R4[0, 7] == 0.0 and R4[1, 7] > 0         # three equal angles: the deviation exactly 0
    R2 = G[("row4", 2)]
    assert R2[0, 0] == 1 and R2[0, 4] == 0 and R2[1, 0] == 2 and R2[1, 4] > 0 and R2[1, 7] == 0   # exactly 1 / exactly 2 neighbors
    W = G[("words", 2)]
    assert sorted(W[:, 9].astype(int).tolist()) == [7, 20, 42, 63, 64, 65, 257]
    bw = nc.batch("words")
    assert W[row_of(bw, 63), 0] == 1 and W[row_of(bw, 63), 1] > 40                        # the 63- and the 65-point box edge to edge
    assert G[("words", 5)][row_of(bw, 257, 1), 0] == 2
    L = G[("long_comb", 5)]
    assert L[0, 9] == 2641 and L[0, 0] == 4 and L[4, 1] == 100.0
    Rg = G[("ring", 5)]
    assert Rg[4, 9] > 512 and Rg[4, 0] == 2 and Rg[0, 0] == 0 and Rg[3, 0] == 0
    La = G[("lattice", 12)]
    st = nr.table(nc.batch("lattice"), 12, with_stats=True)[1]
    assert st["max_candidates"] > 64 and La[:, 0].max() > 32                              # more candidates than a wave has lanes
    T3 = G[("three_images", 5)]
    assert (T3[:16] == T3[16:32]).all() and (T3[:16] == T3[32:]).all() and T3[:, 0].max() >= 2
    P, base = G[("placed", 5)], G[("contacts", 5)]
    assert (P[:, :3] == base[:, :3]).all() and (P[:, 10] == base[:, 10] + nc.FAR_X).all()
    return {"lattice_max_neighbors": int(La[:, 0].max()), "lattice_max_candidates": int(st["max_candidates"]), "comb_contour": int(L[0, 9]), "ring_contour": int(Rg[4, 9])}


def main():
    lib = load()
    store, G = {}, {}
    n_rows = 0
    for name, radii in ((n, c[1]) for n, c in nc.CASES.items()):
        b = nc.batch(name)
        K = contours_of(b)
        for radius in radii:
            T, _ = ref_rows(lib, b, radius)
            assert np.isfinite(T).all(), name
            R = nr.table(b, radius, K)
            assert (R == T).all(), (name, radius, np.argwhere(R != T)[:8], R[R != T][:8], T[R != T][:8])      # every value, bit for bit
            store[f"{name}__r{radius}"] = G[(name, radius)] = T
            n_rows += len(T)
            sd, mean = T[:, 7], T[:, 6]
            assert (sd[sd != 0] >= 1e-3 * np.abs(mean[sd != 0])).all(), (name, radius)
            print(f"{name} R={radius}: {b.n_roi} ROIs in {len(nr.image_ranges(b))} image(s), neighbors max {int(T[:, 0].max())}, "
                  f"touching max {T[:, 1].max():.2f} %")
    every_angle_is_safe(G)
    br = check_branches(G)
    br["rows"] = n_rows
    np.savez_compressed(os.path.join(HERE, "neighbors_reference.npz"), **store)
    json.dump(br, open(os.path.join(HERE, "branches.json"), "w"))
    # the Nyxus path: the stack of API_CASE (one image per tile) at two radii
    I, M = nc.stack(nc.API_CASE)
    b = nc.batch(nc.API_CASE)
    api = {"case": nc.API_CASE, "labels": [int(v) for v in b.roi_label], "tile": np.repeat(np.arange(len(M)), np.diff(b.image_offset.astype(np.int64))).tolist(),
           "columns": nr.NAMES, "numeric": {str(r): G[(nc.API_CASE, r)][:, :9].tolist() for r in (2, 5)}}
    json.dump(api, open(os.path.join(HERE, "api_expected.json"), "w"))
    print(f"recorded {n_rows} rows; branches {br}")
    if os.environ.get("NEIGHBORSREF_TIME"):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import neighbors_probe as probe
        for tag, labs in probe.inputs(n_bench_tiles=int(os.environ.get("NEIGHBORSREF_TILES", "8"))):
            bb = nc.batch_of_images(labs)
            sec = ref_rows(lib, bb, 5)[1]
            print(f"reference NeighborsFeature::manual_reduce, 1 thread, R = 5, {bb.n_roi} ROIs of {tag}: {sec * 1e3:.2f} ms = {sec * 1e3 / len(labs):.3f} ms per image")


def every_angle_is_safe(G):
    """The MODE rounding: every angle between an ROI and ANY of its neighbors (not only the two closest) is an exact integer or at least
    1e-6 from a half-integer.  The neighbor lists are those of the restatement, which equals the recorded values bit for bit."""
    import math
    for (name, radius), T in G.items():
        b = nc.batch(name)
        cen = T[:, 10:12]
        # the neighbors of r: recomputed by the restatement's own pass (cheap: the inputs are small)
        lists = neighbor_lists(b, radius)
        for r, nb in lists.items():
            for q in nb:
                a = nr.direction_angle_deg(cen[r, 0], cen[r, 1], cen[q, 0], cen[q, 1])
                assert a == round(a) or abs(a - math.floor(a) - 0.5) >= 1e-6, (name, radius, r, q, a)


def neighbor_lists(b, radius):
    K = [np.asarray(k, np.int64) + np.array([int(b.origin_x[r]), int(b.origin_y[r])]) for r, k in enumerate(contours_of(b))]
    out = {}
    ox, oy = np.asarray(b.origin_x, np.int64), np.asarray(b.origin_y, np.int64)
    x1, y1 = ox + np.asarray(b.bbox_w, np.int64) - 1, oy + np.asarray(b.bbox_h, np.int64) - 1
    R = int(radius)
    for lo, hi in nr.image_ranges(b):
        for a in range(lo, hi):
            for c in range(a + 1, hi):
                if ox[c] - R > x1[a] + R or x1[c] + R < ox[a] - R or oy[c] - R > y1[a] + R or y1[c] + R < oy[a] - R:
                    continue
                if not len(K[a]) or not len(K[c]):
                    continue
                d = K[a][:, None, :] - K[c][None, :, :]
                if int((d[..., 0] ** 2 + d[..., 1] ** 2).min()) <= R * R:
                    out.setdefault(a, []).append(c)
                    out.setdefault(c, []).append(a)
    return out


if __name__ == "__main__":
    main()
