#!/usr/bin/env python3
"""Generates tests/golden/caliper/caliper_reference.npz and api_expected.json: the output of the reference's own ConvexHullFeature +
CaliperFeretFeature + CaliperMartinFeature + CaliperNassensteinFeature on the inputs of tests/caliper_cases.py, every ROI at its
absolute position.  Only DATA is stored (20 doubles per ROI, the hull vertices, the per-angle diameters); the inputs are rebuilt from
seeds by tests/caliper_cases.py.

The reference classes are compiled OUTSIDE the repository: ref_caliper_driver.cpp (own code, next to this file) against the
reference sources where they lie, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    REF=/root/reference/src/nyx; W=$(mktemp -d)
    for f in features/caliper_feret features/caliper_martin features/caliper_nassenstein features/convex_hull_nontriv \\
             features/rotation common_stats; do
        g++ -std=c++20 -O2 -fPIC -w -I/opt/conda/include -c $REF/$f.cpp -o $W/$(basename $f).o; done
    g++ -std=c++20 -O2 -fPIC -shared -w -I$REF -Iinclude -I/opt/conda/include -o $W/libcalref.so \\
        tests/golden/caliper/ref_caliper_driver.cpp $W/*.o \\
        $(find oracle/_ref/obj -name '*.o') /usr/lib/x86_64-linux-gnu/libtiff.so.5 -lpthread
    CALREF_SO=$W/libcalref.so python tests/golden/caliper/make_caliper_golden.py

The generator refuses fixtures on which a mode could flip under a last-bit difference of the host libm.  The test is direct
(caliper_ref.libm_sensitive, on the restatement, which this run also pins to the driver's per-angle values bit for bit): every
sin / cos of the table is moved by one unit in the last place, in all four sign combinations, and an ROI whose angles or modes
change is refused.  A refused ROI of the random part is answered by another seed (caliper_cases.RANDOM_SEED); a refused named
shape stops the run.  The coarser condition "a per-angle diameter within 1e-4 of an integer without being that integer" is
counted and printed but cannot be a refusal: the reference's angle is a float, cos(90 deg) is -4.4e-8 there, and EVERY lattice
shape -- the rectangles, the lines, the 2 x 2 block -- has an integer extent that comes out as 2.0000002 or 6.9999995 at 90 or
180 degrees.  Such a value is a fixed float of the reference, not a libm accident: it moves only if a rotated coordinate sits
within 1e-16 of a float rounding boundary, which is what the direct test looks for.

With CALREF_TIME=1 it also times the reference classes on 16 CPU threads over the benchmark's ROIs (bench.py's tile batch) and
prints the seconds per class.

The reference's Python package is not built here, so api_expected.json holds driver-recorded tables with the reference's
user-facing column names (featureset.cpp UserFacingFeatureNames).
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
from tests import caliper_cases, caliper_ref  # noqa: E402


def load():
    lib = C.CDLL(os.environ["CALREF_SO"])
    lib.calref_batch.restype = C.c_int
    lib.calref_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, soft_nan=0.0, n_threads=1, timed=False):
    cb = b.c_struct()
    n = b.n_roi
    out = np.zeros((n, 20))
    hn = np.zeros(n, np.int32)
    cap = int(2 * b.bbox_w.astype(np.int64).sum() + 16)
    hxy = np.zeros((cap, 2), np.int32)
    pa = np.zeros((n, 3, 19))
    fa = np.zeros((n, 19))
    sec = np.zeros(4)
    ox = b.origin_x if b.origin_x is not None else np.zeros(n, np.uint32)
    oy = b.origin_y if b.origin_y is not None else np.zeros(n, np.uint32)
    rc = lib.calref_batch(C.byref(cb), ox.ctypes.data, oy.ctypes.data, soft_nan, n_threads, out.ctypes.data, hn.ctypes.data, hxy.ctypes.data,
                          cap, pa.ctypes.data, fa.ctypes.data, sec.ctypes.data if timed else None)
    assert rc == 0, rc
    off = np.concatenate([[0], np.cumsum(hn)]).astype(np.int64)
    return out, off, hxy[:off[-1]].copy(), pa, fa, sec


def main():
    lib = load()
    store = {}
    refused = {}
    for name in caliper_cases.CASES:
        b = caliper_cases.batch(name)
        T, off, pts, pa, fa, _ = ref_rows(lib, b)
        assert np.isfinite(T).all(), name
        bad = caliper_ref.libm_sensitive(b)
        near = caliper_ref.near_integer(b)
        refused[name] = bad
        # the restatement's per-angle diameters are the driver's, bit for bit (the refusal above rests on them)
        px = b.px_offset.astype(np.int64)
        tab = caliper_ref.sincos_table()
        for r in range(b.n_roi):
            Fr, Mr, Nr = caliper_ref.diameters(b.x[px[r]:px[r + 1]], b.y[px[r]:px[r + 1]], b.origin_x[r], b.origin_y[r], tab)
            for got, want in (([d for _, d in Fr], pa[r, 0]), (Mr, pa[r, 1]), (Nr, pa[r, 2])):
                w = want[~np.isnan(want)]
                assert len(got) == len(w) and all(g == v for g, v in zip(got, w)), (name, r, got, list(w))
        store[f"{name}__table"] = T
        store[f"{name}__hull_offset"], store[f"{name}__hull_points"] = off, pts
        store[f"{name}__feret"], store[f"{name}__martin"], store[f"{name}__nassenstein"] = pa[:, 0], pa[:, 1], pa[:, 2]
        print(f"{name}: {b.n_roi} ROIs, max pixels {int(np.diff(px).max())}, hull vertices {np.diff(off).min()}..{np.diff(off).max()}, "
              f"refused (angles / modes move with the last bit of sin / cos): {bad}; ROIs with a diameter within 1e-4 of an integer: {len(near)}")
    n_named = {"degenerate": 7, "shapes": 8, "placed": 24, "wide": 12, "tile": 0}
    for name, bad in refused.items():
        assert not [r for r in bad if r < n_named[name]], f"a named shape of {name} is refused: {bad}"
        assert not bad, f"{name}: ROIs {bad} refused -- choose another caliper_cases.RANDOM_SEED"
    print("refused candidates:", {k: len(v) for k, v in refused.items()})
    b = caliper_cases.batch("degenerate")
    store["degenerate_softnan__table"] = ref_rows(lib, b, soft_nan=-7.5)[0]
    assert (store["degenerate_softnan__table"][0] == -7.5).all() and (store["degenerate__table"][0] == 0.0).all()
    # the reason the origin exists: at least one column of at least one shape differs between two placements in the reference itself
    P = store["placed__table"].reshape(3, 8, 20)
    differs = [(s, int((P[0, s] != P[k, s]).sum())) for s in range(8) for k in (1, 2) if (P[0, s] != P[k, s]).any()]
    rel = np.abs(P[1:] - P[0]) / np.maximum(np.abs(P[0]), 1e-300)
    print(f"placed: shapes whose rows differ between placements (shape, columns): {differs}; largest relative difference {np.nanmax(rel):.3e}")
    assert differs, "the reference shows no dependence on the placement"
    np.savez_compressed(os.path.join(HERE, "caliper_reference.npz"), **store)
    labels = [int(r["label"]) for r in caliper_cases.tile_rois()]
    T = store["tile__table"]
    N = caliper_ref.NAMES
    pick = ["STAT_MARTIN_DIAM_MEDIAN", "MAX_FERET_ANGLE", "STAT_NASSENSTEIN_DIAM_MIN", "STAT_FERET_DIAM_MAX"]
    order = sorted(pick, key=N.index)
    api = {"inten_dtype": "uint32", "labels": labels,
           "cases": {"four_codes": {"features": pick, "columns": order, "numeric": T[:, [N.index(c) for c in order]].tolist()},
                     "all_twenty": {"features": list(N), "columns": list(N), "numeric": T.tolist()}}}
    json.dump(api, open(os.path.join(HERE, "api_expected.json"), "w"))
    if os.environ.get("CALREF_TIME"):
        from tests import synth
        bb = synth.tile_batch(0)
        reps = max(1, 196_000 // bb.n_roi)
        sec = ref_rows(lib, bb, n_threads=16, timed=True)[5]
        print(f"reference classes, 16 threads, {bb.n_roi} ROIs of the benchmark tile: hull {sec[0] * 1e3:.2f} ms, Feret {sec[1] * 1e3:.2f} ms, "
              f"Martin {sec[2] * 1e3:.2f} ms, Nassenstein {sec[3] * 1e3:.2f} ms; x {reps} for 196 k ROIs")


if __name__ == "__main__":
    main()
