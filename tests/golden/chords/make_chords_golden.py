#!/usr/bin/env python3
"""Generates tests/golden/chords/chords_reference.npz and api_expected.json: the output of the reference's own ChordsFeature on the
inputs of tests/chords_cases.py, every ROI at its absolute position and in its cloud order.  Only DATA is stored (16 doubles per
ROI; per angle the longest chord, the number of chords and their sum); the inputs are rebuilt from seeds by tests/chords_cases.py.

The reference class is compiled OUTSIDE the repository: ref_chords_driver.cpp (own code, next to this file) against the reference
sources where they lie, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    REF=/root/reference/src/nyx; W=$(mktemp -d)
    for f in features/chords features/chords_nontriv features/rotation; do
        g++ -std=c++20 -O2 -fPIC -w -I/opt/conda/include -c $REF/$f.cpp -o $W/$(basename $f).o; done
    g++ -std=c++20 -O2 -fPIC -shared -w -I$REF -Iinclude -I/opt/conda/include -o $W/libchordsref.so \\
        tests/golden/chords/ref_chords_driver.cpp $W/*.o \\
        $(find oracle/_ref/obj -name '*.o') /usr/lib/x86_64-linux-gnu/libtiff.so.5 -lpthread
    CHORDSREF_SO=$W/libchordsref.so python tests/golden/chords/make_chords_golden.py

The generator refuses fixtures on which a chord could change under a last-bit difference of the host libm.  The test is direct
(chords_ref.libm_sensitive, on the restatement, which this run also pins to the driver's per-angle values): every sin / cos of the
table is moved by one unit in the last place, in all four sign combinations, and an ROI of which any pixel changes its cell at any
angle is refused.  A refused ROI of the random part is answered by another seed (chords_cases.RANDOM_SEED); a refused named shape
stops the run.

With CHORDSREF_TIME=1 it also times the reference class on 16 CPU threads over the benchmark's ROIs (bench.py's tile batch) and
over a heavy-tailed batch, and prints the seconds.

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
from tests import chords_cases, chords_ref  # noqa: E402


def load():
    lib = C.CDLL(os.environ["CHORDSREF_SO"])
    lib.chordsref_batch.restype = C.c_int
    lib.chordsref_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, soft_nan=0.0, n_threads=1, timed=False, per_angle=True):
    cb = b.c_struct()
    n = b.n_roi
    out = np.zeros((n, 16))
    pa = np.zeros((n, 3, 20), np.int64)
    sec = np.zeros(1)
    ox = b.origin_x if b.origin_x is not None else np.zeros(n, np.uint32)
    oy = b.origin_y if b.origin_y is not None else np.zeros(n, np.uint32)
    rc = lib.chordsref_batch(C.byref(cb), ox.ctypes.data, oy.ctypes.data, soft_nan, n_threads, out.ctypes.data,
                             pa.ctypes.data if per_angle else None, sec.ctypes.data if timed else None)
    assert rc == 0, rc
    return out, pa, sec[0]


def main():
    lib = load()
    store = {}
    refused = {}
    for name in chords_cases.CASES:
        b = chords_cases.batch(name)
        T, pa, _ = ref_rows(lib, b)
        assert np.isfinite(T).all(), name
        bad = chords_ref.libm_sensitive(b)
        refused[name] = bad
        # the restatement's per-angle values are the driver's (the refusal above rests on them), and so are its rows
        P = chords_ref.batch_per_angle(b)
        for r in range(b.n_roi):
            mx, cnt, sm = chords_ref.summary(P[r])
            assert (mx == pa[r, 0]).all() and (cnt == pa[r, 1]).all() and (sm == pa[r, 2]).all(), (name, r)
        R = chords_ref.table(b)
        assert (R == T).all(), (name, np.argwhere(R != T)[:5])
        store[f"{name}__table"] = T
        store[f"{name}__max"], store[f"{name}__count"], store[f"{name}__sum"] = pa[:, 0], pa[:, 1], pa[:, 2]
        px = b.px_offset.astype(np.int64)
        print(f"{name}: {b.n_roi} ROIs, max pixels {int(np.diff(px).max())}, chords per ROI {pa[:, 1].sum(1).min()}..{pa[:, 1].sum(1).max()}, "
              f"rows of zeros {int((T == 0).all(1).sum())}, refused (a cell moves with the last bit of sin / cos): {bad}")
    for name, bad in refused.items():
        assert not [r for r in bad if r < chords_cases.N_NAMED[name]], f"a named shape of {name} is refused: {bad}"
        assert not bad, f"{name}: ROIs {bad} refused -- choose another chords_cases.RANDOM_SEED"
    b = chords_cases.batch("degenerate")
    store["degenerate_softnan__table"] = ref_rows(lib, b, soft_nan=-7.5)[0]
    # the reason the family reads the origin: at least one column of at least one shape differs between two placements in the reference
    P = store["placed__table"].reshape(3, 8, 16)
    differs = [(s, int((P[0, s] != P[k, s]).sum())) for s in range(8) for k in (1, 2) if (P[0, s] != P[k, s]).any()]
    print(f"placed: shapes whose rows differ between placements (shape, columns): {differs}")
    assert differs, "the reference shows no dependence on the placement"
    Z = store["zeros__table"]
    print(f"zeros: the collision ROI in cloud order and reversed differ in {int((Z[2] != Z[3]).sum())} columns")
    np.savez_compressed(os.path.join(HERE, "chords_reference.npz"), **store)
    labels = [int(r["label"]) for r in chords_cases.tile_rois()]
    T = store["tile__table"]
    N = chords_ref.NAMES
    pick = ["ALLCHORDS_MEDIAN", "MAXCHORDS_MAX", "ALLCHORDS_STDDEV", "MAXCHORDS_MIN_ANG"]
    order = sorted(pick, key=N.index)
    api = {"inten_dtype": "uint32", "labels": labels,
           "cases": {"four_codes": {"features": pick, "columns": order, "numeric": T[:, [N.index(c) for c in order]].tolist()},
                     "all_sixteen": {"features": list(N), "columns": list(N), "numeric": T.tolist()}}}
    json.dump(api, open(os.path.join(HERE, "api_expected.json"), "w"))
    if os.environ.get("CHORDSREF_TIME"):
        from tests import radial_cases, synth
        from nyxus_amd import _abi
        bb = synth.tile_batch(0)
        sec = ref_rows(lib, bb, n_threads=16, timed=True, per_angle=False)[2]
        print(f"reference class, 16 threads, {bb.n_roi} ROIs of the benchmark tile: {sec * 1e3:.2f} ms = {sec * 1e9 / bb.n_roi:.0f} ns per ROI")
        hb = _abi.batch_from_rois(radial_cases.heavy())
        sec = ref_rows(lib, hb, n_threads=16, timed=True, per_angle=False)[2]
        print(f"reference class, 16 threads, {hb.n_roi} ROIs of the heavy-tailed batch: {sec * 1e3:.2f} ms = {sec * 1e9 / hb.n_roi:.0f} ns per ROI")


if __name__ == "__main__":
    main()
