#!/usr/bin/env python3
"""Generates tests/golden/circle/circle_reference.npz and api_expected.json: the output of the reference's own
EnclosingInscribingCircumscribingCircleFeature and GeodeticLengthThicknessFeature (behind BasicMorphologyFeatures and ContourFeature,
their dependencies) on the inputs of tests/circle_cases.py, every ROI at its ABSOLUTE position.  Only DATA is stored (per ROI the
five columns, PERIMETER, CENTROID_X, CENTROID_Y, the contour length and which branch of SqRootTmp < 0 was taken); the inputs are
rebuilt from seeds by tests/circle_cases.py.

The reference classes are compiled OUTSIDE the repository: ref_circle_driver.cpp (own code, next to this file) against the reference
sources where they lie, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    REF=/root/reference/src/nyx; W=$(mktemp -d)
    for f in features/circle features/geo_len_thickness features/basic_morphology; do
        g++ -std=c++20 -O2 -fPIC -w -I/opt/conda/include -c $REF/$f.cpp -o $W/$(basename $f).o; done
    g++ -std=c++20 -O2 -fPIC -shared -w -I$REF -Iinclude -I/opt/conda/include -o $W/libcircleref.so \\
        tests/golden/circle/ref_circle_driver.cpp $W/*.o \\
        $(find oracle/_ref/obj -name '*.o') /usr/lib/x86_64-linux-gnu/libtiff.so.5 -lpthread
    CIRCLEREF_SO=$W/libcircleref.so python tests/golden/circle/make_circle_golden.py

Every value of every ROI is compared, bit for bit, with tests/circle_ref.py before it is stored: there is no `compared` mask.  The
generator also asserts that both branches of SqRootTmp < 0 occur (compact shapes clamp it, needles and combs do not), that the
contours of circle_cases.WORD_BOXES have the lengths their names say, and that the long comb's contour exceeds the LDS bound.

With CIRCLEREF_TIME=1 it also times the two reference classes on 16 CPU threads over the benchmark's ROIs (bench.py's tile batch)
and over a heavy-tailed batch, and prints the seconds.

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
from tests import circle_cases, circle_ref  # noqa: E402


def load():
    lib = C.CDLL(os.environ["CIRCLEREF_SO"])
    lib.circleref_batch.restype = C.c_int
    lib.circleref_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, soft_nan=0.0, n_threads=1, timed=False):
    cb = b.c_struct()
    n = b.n_roi
    out = np.zeros((n, 8))
    nk = np.zeros(n, np.int32)
    sec = np.zeros(2)
    ox = b.origin_x if b.origin_x is not None else np.zeros(n, np.uint32)
    oy = b.origin_y if b.origin_y is not None else np.zeros(n, np.uint32)
    rc = lib.circleref_batch(C.byref(cb), ox.ctypes.data, oy.ctypes.data, soft_nan, n_threads, out.ctypes.data, nk.ctypes.data,
                             sec.ctypes.data if timed else None)
    assert rc == 0, rc
    return out, nk, sec


def main():
    lib = load()
    store = {}
    clamped_any, free_any = False, False
    for name in circle_cases.CASES:
        b = circle_cases.batch(name)
        T, nk, _ = ref_rows(lib, b)
        assert np.isfinite(T).all(), name
        R, flags = circle_ref.table(b, with_flags=True)
        assert (R == T).all(), (name, np.argwhere(R != T)[:8], R[R != T][:8], T[R != T][:8])      # every value, bit for bit
        store[f"{name}__table"], store[f"{name}__n_contour"], store[f"{name}__clamped"] = T, nk, flags
        clamped_any |= bool(flags.any())
        free_any |= bool((~flags & (nk > 0)).any())
        print(f"{name}: {b.n_roi} ROIs, contour lengths {nk.tolist() if len(nk) <= 40 else (int(nk.min()), int(nk.max()))}, "
              f"SqRootTmp clamped in {int(flags.sum())}")
    assert clamped_any and free_any, "both branches of SqRootTmp < 0 must occur"
    assert store["small__n_contour"].tolist() == [0, 0, 3, 2, 3, 0]
    assert store["words__n_contour"].tolist() == sorted(circle_cases.WORD_BOXES)
    assert store["long_comb__n_contour"][0] > circle_cases.CONTOUR_LDS
    b = circle_cases.batch("shapes")
    store["shapes_softnan__table"] = ref_rows(lib, b, soft_nan=-7.5)[0]
    np.savez_compressed(os.path.join(HERE, "circle_reference.npz"), **store)
    labels = [int(r["label"]) for r in circle_cases.tile_rois()]
    T = store["tile__table"][:, :5]
    N = circle_ref.NAMES
    pick = ["GEODETIC_LENGTH", "DIAMETER_INSCRIBING_CIRCLE"]
    order = sorted(pick, key=N.index)
    idx = [N.index(c) for c in order]
    api = {"inten_dtype": "uint32", "labels": labels,
           "cases": {"two_codes": {"features": pick, "columns": order, "numeric": T[:, idx].tolist()},
                     "all_five": {"features": list(N), "columns": list(N), "numeric": T.tolist()}}}
    json.dump(api, open(os.path.join(HERE, "api_expected.json"), "w"))
    if os.environ.get("CIRCLEREF_TIME"):
        from tests import radial_cases, synth
        from nyxus_amd import _abi
        for tag, bb in (("the benchmark tile", synth.tile_batch(0)), ("the heavy-tailed batch", _abi.batch_from_rois(radial_cases.heavy()))):
            sec = ref_rows(lib, bb, n_threads=16, timed=True)[2]
            for k, cls in enumerate(("EnclosingInscribingCircumscribingCircleFeature", "GeodeticLengthThicknessFeature")):
                print(f"reference {cls}, 16 threads, {bb.n_roi} ROIs of {tag}: {sec[k] * 1e3:.2f} ms = {sec[k] * 1e9 / bb.n_roi:.0f} ns per ROI")


if __name__ == "__main__":
    main()
