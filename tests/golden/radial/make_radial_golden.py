#!/usr/bin/env python3
"""Generates tests/golden/radial/radial_reference.npz: the output of the reference's own ContourFeature +
RadialDistributionFeature on the inputs of tests/radial_cases.py.  Only DATA is stored (24 doubles per ROI, the centre's
squared radius, the contour length); the inputs are rebuilt from seeds by tests/radial_cases.py.

The reference classes are compiled OUTSIDE the repository: ref_radial_driver.cpp (own code, next to this file) against the
reference sources where they lie, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    REF=/root/reference/src/nyx; W=$(mktemp -d)
    g++ -std=c++20 -O2 -fPIC -w -I/opt/conda/include -c $REF/features/radial_distribution.cpp -o $W/radial_distribution.o
    g++ -std=c++20 -O2 -fPIC -shared -w -I$REF -Iinclude -I/opt/conda/include -o $W/libradref.so \\
        tests/golden/radial/ref_radial_driver.cpp $W/radial_distribution.o $(find oracle/_ref/obj -name '*.o') \\
        /usr/lib/x86_64-linux-gnu/libtiff.so.5 -lpthread
    RADREF_SO=$W/libradref.so python tests/golden/radial/make_radial_golden.py

The generator refuses inputs on which the reference itself is undefined (a centre with max_sqdist == 0: division by zero and a
NaN converted to int), so that no test has a row to skip, and checks the 8 x 8 shape2d ROI against the reference's own
regression vector (tests/test_2d_radial_regression.h:20-33, stored in reference_regression.json).

The reference's Python package is not built in this container, so no Nyxus.featurize() DataFrame of the reference is captured
for this family; api_expected.json holds driver-recorded tables with the column names the reference's header code produces
(output_2_buffer.cpp:364-411).
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
from nyxus_amd import _abi  # noqa: E402
from tests import radial_cases  # noqa: E402


def ref_rows(lib, b, n_threads=1):
    cb = b.c_struct()
    out = np.zeros((b.n_roi, 24))
    dst2 = np.zeros(b.n_roi)
    nk = np.zeros(b.n_roi, np.int32)
    sec = np.zeros(2)
    rc = lib.radref_batch(C.byref(cb), n_threads, out.ctypes.data, dst2.ctypes.data, nk.ctypes.data, sec.ctypes.data)
    assert rc == 0, rc
    return out, dst2, nk, sec


def main():
    lib = C.CDLL(os.environ["RADREF_SO"])
    lib.radref_batch.restype = C.c_int
    lib.radref_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    store = {}
    for name in radial_cases.CASES:
        b = radial_cases.batch(name)
        T, d2, nk, _ = ref_rows(lib, b)
        assert not (d2 == 0).any(), (name, np.nonzero(d2 == 0)[0])           # the reference is defined on every input
        assert np.isfinite(T).all(), name
        assert ((d2 < 0) == (nk == 0)).all(), name
        store[f"{name}__table"], store[f"{name}__dst2"], store[f"{name}__n_contour"] = T, d2, nk
        print(f"{name}: {b.n_roi} ROIs, max pixels {int(np.diff(b.px_offset.astype(np.int64)).max())}, contour points {nk.min()}..{nk.max()}, "
              f"without contour {(nk == 0).sum()}")
    # the reference's own regression vector for the shape2d ROI (its test compares with an absolute 1e-9)
    reg = json.load(open(os.path.join(HERE, "reference_regression.json")))
    want = np.array(reg["FRAC_AT_D"] + reg["MEAN_FRAC"] + reg["RADIAL_CV"])
    assert np.abs(store["shape2d__table"][0] - want).max() <= 1e-9, store["shape2d__table"][0] - want
    assert store["special__n_contour"].min() == 0 and store["heavy__n_contour"].max() > 2048
    np.savez_compressed(os.path.join(HERE, "radial_reference.npz"), **store)
    # Nyxus.featurize() expectations (driver-recorded): the tile's rows under two feature requests, with the reference's column names
    it, lab = radial_cases.tile()
    labels = [int(r["label"]) for r in radial_cases.tile_rois()]
    T = store["tile__table"]
    cols = lambda code: [f"{code}_{i}" for i in range(8)]
    api = {"inten_dtype": "uint32", "labels": labels,
           "cases": {"frac_at_d_and_radial_cv": {"features": ["RADIAL_CV", "FRAC_AT_D"], "columns": cols("FRAC_AT_D") + cols("RADIAL_CV"),
                                                  "numeric": np.hstack([T[:, 0:8], T[:, 16:24]]).tolist()},
                     "all_three": {"features": ["FRAC_AT_D", "MEAN_FRAC", "RADIAL_CV"], "columns": cols("FRAC_AT_D") + cols("MEAN_FRAC") + cols("RADIAL_CV"),
                                   "numeric": T.tolist()}}}
    json.dump(api, open(os.path.join(HERE, "api_expected.json"), "w"))


if __name__ == "__main__":
    main()
