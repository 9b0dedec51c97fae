#!/usr/bin/env python3
"""Generates tests/golden/erosion/erosion_reference.npz and api_expected.json: the output of the reference's own
EllipseFittingFeature (behind BasicMorphologyFeatures, its dependency) and ErosionPixelsFeature (behind the aux_min == aux_max skip of
its driver) on the inputs of tests/erosion_cases.py.  Only DATA is stored (8 doubles per ROI and the `compared` mask); the inputs are
rebuilt from seeds by tests/erosion_cases.py.

The reference classes are compiled OUTSIDE the repository: ref_erosion_driver.cpp (own code, next to this file) against the reference
sources where they lie, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    REF=/root/reference/src/nyx; W=$(mktemp -d)
    for f in features/erosion features/ellipse_fitting features/basic_morphology; do
        g++ -std=c++20 -O2 -fPIC -w -I/opt/conda/include -c $REF/$f.cpp -o $W/$(basename $f).o; done
    g++ -std=c++20 -O2 -fPIC -shared -w -I$REF -Iinclude -I/opt/conda/include -o $W/liberosionref.so \\
        tests/golden/erosion/ref_erosion_driver.cpp $W/*.o \\
        $(find oracle/_ref/obj -name '*.o') /usr/lib/x86_64-linux-gnu/libtiff.so.5 -lpthread
    EROSIONREF_SO=$W/liberosionref.so python tests/golden/erosion/make_erosion_golden.py

Which ellipse values are compared: for an axis-symmetric shape the reference's uxy and `common` are rounding noise about an exact
zero, so its ORIENTATION can be a noisy +-90 and its ECCENTRICITY the root of noise.  The generator computes uxx, uyy, uxy and common
exactly (erosion_ref.exact, Fractions) and stores a boolean mask per ROI and column (erosion_ref.compared): ORIENTATION is compared
where |uxy| >= 1e-6 (uxx + uyy), or where uxy is exactly 0 and the reference returned exactly 0.0 or 90.0; ECCENTRICITY where
common >= 1e-6 (uxx + uyy); the other columns always.  (fp64 sum noise is about 1e-13 relative; amplified by 1e6 it stays two
orders under parity.REL_TOL.)  The cap: no shape of erosion_cases.ASYMMETRIC has a masked value, and at most 10 % of the seeded ROIs
of any case have one; a refused seeded ROI is answered by another erosion_cases.RANDOM_SEED.

With EROSIONREF_TIME=1 it also times the two reference classes on 16 CPU threads over the benchmark's ROIs (bench.py's tile batch)
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
from tests import erosion_cases, erosion_ref, parity  # noqa: E402


def load():
    lib = C.CDLL(os.environ["EROSIONREF_SO"])
    lib.erosionref_batch.restype = C.c_int
    lib.erosionref_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, soft_nan=0.0, n_threads=1, timed=False):
    cb = b.c_struct()
    n = b.n_roi
    out = np.zeros((n, 8))
    sec = np.zeros(2)
    ox = b.origin_x if b.origin_x is not None else np.zeros(n, np.uint32)
    oy = b.origin_y if b.origin_y is not None else np.zeros(n, np.uint32)
    rc = lib.erosionref_batch(C.byref(cb), ox.ctypes.data, oy.ctypes.data, soft_nan, n_threads, out.ctypes.data, sec.ctypes.data if timed else None)
    assert rc == 0, rc
    return out, sec


def compared_of(b, T):
    return np.array([erosion_ref.compared(x, y, T[r, 4]) for r, x, y in erosion_ref.rois_of(b)]).reshape(b.n_roi, 8)


def check_cap(name, M):
    """The cap on masked values (also asserted by tests/test_erosion_cpu.py)."""
    masked = ~M.all(1)
    bad = [r for r in erosion_cases.ASYMMETRIC[name] if masked[r]]
    assert not bad, f"{name}: asymmetric shapes {bad} have a masked value"
    rnd = erosion_cases.random_indices(name, len(M))
    if rnd:
        k = int(masked[rnd].sum())
        assert 10 * k <= len(rnd), f"{name}: {k} of {len(rnd)} seeded ROIs have a masked value -- choose another erosion_cases.RANDOM_SEED"


def main():
    lib = load()
    store = {}
    for name in erosion_cases.CASES:
        b = erosion_cases.batch(name)
        T, _ = ref_rows(lib, b)
        assert np.isfinite(T).all(), name
        M = compared_of(b, T)
        check_cap(name, M)
        R = erosion_ref.table(b)
        assert (R[:, 6:] == T[:, 6:]).all(), (name, np.argwhere(R[:, 6:] != T[:, 6:])[:5])          # the erosion columns bit for bit
        assert (T[:, 7] == 0).all()
        ok = np.abs(R[:, :6] - T[:, :6]) <= parity.REL_TOL * np.abs(T[:, :6])
        assert (ok | ~M[:, :6]).all(), (name, np.argwhere(~(ok | ~M[:, :6]))[:5])
        assert ((T[:, 3] >= 0) & (T[:, 3] <= 1) & (np.abs(T[:, 4]) <= 90)).all() and ((R[:, 3] >= 0) & (R[:, 3] <= 1) & (np.abs(R[:, 4]) <= 90)).all()
        store[f"{name}__table"], store[f"{name}__compared"] = T, M
        px = b.px_offset.astype(np.int64)
        err = np.where(M[:, :6], np.abs(R[:, :6] - T[:, :6]) / np.maximum(np.abs(T[:, :6]), 1e-300), 0).max()
        print(f"{name}: {b.n_roi} ROIs, max pixels {int(np.diff(px).max())}, EROSIONS_2_VANISH {sorted(set(T[:, 6].astype(int)))}, "
              f"masked ORIENTATION {int((~M[:, 4]).sum())}, masked ECCENTRICITY {int((~M[:, 3]).sum())}, "
              f"largest relative difference of the restatement on compared values {err:.3g}")
    b = erosion_cases.batch("shapes")
    store["shapes_softnan__table"] = ref_rows(lib, b, soft_nan=-7.5)[0]
    np.savez_compressed(os.path.join(HERE, "erosion_reference.npz"), **store)
    labels = [int(r["label"]) for r in erosion_cases.tile_rois()]
    T, M = store["tile__table"], store["tile__compared"]
    N = erosion_ref.NAMES
    pick = ["EROSIONS_2_VANISH", "ROUNDNESS", "MAJOR_AXIS_LENGTH", "ORIENTATION"]
    order = sorted(pick, key=N.index)
    idx = [N.index(c) for c in order]
    api = {"inten_dtype": "uint32", "labels": labels,
           "cases": {"four_codes": {"features": pick, "columns": order, "numeric": T[:, idx].tolist(), "compared": M[:, idx].tolist()},
                     "all_eight": {"features": list(N), "columns": list(N), "numeric": T.tolist(), "compared": M.tolist()}}}
    json.dump(api, open(os.path.join(HERE, "api_expected.json"), "w"))
    if os.environ.get("EROSIONREF_TIME"):
        from tests import radial_cases, synth
        from nyxus_amd import _abi
        for tag, bb in (("the benchmark tile", synth.tile_batch(0)), ("the heavy-tailed batch", _abi.batch_from_rois(radial_cases.heavy()))):
            sec = ref_rows(lib, bb, n_threads=16, timed=True)[1]
            for k, cls in enumerate(("EllipseFittingFeature", "ErosionPixelsFeature")):
                print(f"reference {cls}, 16 threads, {bb.n_roi} ROIs of {tag}: {sec[k] * 1e3:.2f} ms = {sec[k] * 1e9 / bb.n_roi:.0f} ns per ROI")


if __name__ == "__main__":
    main()
