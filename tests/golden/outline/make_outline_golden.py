#!/usr/bin/env python3
"""Generates tests/golden/outline/outline_reference.npz and api_expected.json: the output of the reference's own ContourFeature +
FractalDimensionFeature + EulerNumberFeature + RoiRadiusFeature on the inputs of tests/outline_cases.py.  Only DATA is stored (six
doubles per ROI, the contour length, the shifted-grid box counts of the small ROIs); the inputs are rebuilt from seeds by
tests/outline_cases.py.

The reference classes are compiled OUTSIDE the repository: ref_outline_driver.cpp (own code, next to this file) against the
reference sources where they lie, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    REF=/root/reference/src/nyx; W=$(mktemp -d)
    for f in fractal_dim euler_number roi_radius; do
        g++ -std=c++20 -O2 -fPIC -w -I/opt/conda/include -c $REF/features/$f.cpp -o $W/$f.o; done
    g++ -std=c++20 -O2 -fPIC -shared -w -I$REF -Iinclude -I/opt/conda/include -o $W/liboutref.so \\
        tests/golden/outline/ref_outline_driver.cpp $W/fractal_dim.o $W/euler_number.o $W/roi_radius.o \\
        $(find oracle/_ref/obj -name '*.o') /usr/lib/x86_64-linux-gnu/libtiff.so.5 -lpthread
    OUTREF_SO=$W/liboutref.so python tests/golden/outline/make_outline_golden.py

The generator refuses inputs on which the reference itself is undefined: an ROI whose merged contour is a single point (the hill
descent of Pixel2::min_sqdist converts 1 / log(1) to int).  The driver does not run RoiRadiusFeature there; the generator asserts
that no case holds such an ROI, so that no test has a value to skip.

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
from tests import outline_cases  # noqa: E402


def load():
    lib = C.CDLL(os.environ["OUTREF_SO"])
    lib.outref_batch.restype = C.c_int
    lib.outref_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, n_threads=1, timed=False):
    cb = b.c_struct()
    out = np.zeros((b.n_roi, 6))
    nk = np.zeros(b.n_roi, np.int32)
    bc = np.zeros((b.n_roi, 5, 4), np.int32)
    sec = np.zeros(4)
    rc = lib.outref_batch(C.byref(cb), n_threads, out.ctypes.data, nk.ctypes.data, bc.ctypes.data, sec.ctypes.data if timed else None)
    assert rc == 0, rc
    return out, nk, bc, sec


def main():
    lib = load()
    store = {}
    for name in outline_cases.CASES:
        b = outline_cases.batch(name)
        T, nk, bc, _ = ref_rows(lib, b)
        assert not (nk == 1).any(), (name, np.nonzero(nk == 1)[0])            # the reference is defined on every input
        assert np.isfinite(T).all(), name
        store[f"{name}__table"], store[f"{name}__n_contour"], store[f"{name}__box_counts"] = T, nk, bc
        print(f"{name}: {b.n_roi} ROIs, max pixels {int(np.diff(b.px_offset.astype(np.int64)).max())}, contour points {nk.min()}..{nk.max()}, "
              f"Euler {T[:, 2].min():.0f}..{T[:, 2].max():.0f}")
    s = store["small__table"]
    assert s[2, 2] == 1 and s[6, 2] == 0 and s[7, 2] == -1                   # diagonal pair: one object; ring; plate with two holes
    assert list(store["small__n_contour"][9:13]) == [3, 4, 7, 8]
    assert store["heavy__n_contour"].max() > 2048
    np.savez_compressed(os.path.join(HERE, "outline_reference.npz"), **store)
    labels = [int(r["label"]) for r in outline_cases.tile_rois()]
    T = store["tile__table"]
    N = outline_cases.NAMES
    api = {"inten_dtype": "uint32", "labels": labels,
           "cases": {"radius_and_euler": {"features": ["ROI_RADIUS_MAX", "EULER_NUMBER", "ROI_RADIUS_MEAN"], "columns": [N[2], N[3], N[4]],
                                          "numeric": T[:, [2, 3, 4]].tolist()},
                     "all_six": {"features": list(N), "columns": list(N), "numeric": T.tolist()}}}
    json.dump(api, open(os.path.join(HERE, "api_expected.json"), "w"))


if __name__ == "__main__":
    main()
