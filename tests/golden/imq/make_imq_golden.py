#!/usr/bin/env python3
"""Generates tests/golden/imq/imq_reference.npz and api_expected.json: the output of the reference's own FocusScoreFeature and
SaturationFeature on the inputs of tests/imq_cases.py.  Only DATA is stored (per ROI the four values as the classes leave them); the
inputs are rebuilt from seeds by tests/imq_cases.py.  published.json (the fixture and the four values the reference's tests carry) is not
generated: it is transcribed.

The reference classes are compiled OUTSIDE the repository, into a temporary directory: ref_imq_driver.cpp (own code, next to this file)
and features/focus_score.cpp, features/saturation.cpp of the reference where they lie, linked with the objects oracle/Makefile leaves in
oracle/_ref/obj:

    python tests/golden/imq/make_imq_golden.py          # REF=<reference>/src/nyx overrides the place of the reference sources

Before anything is stored, tests/imq_ref.py must equal the recording bit for bit on the two saturation columns and within parity.REL_TOL
on the two focus columns, and the published values must hold on the recording.  A box with a side of 1 is never handed to the reference:
its LOCAL_FOCUS_SCORE loop does not end (the driver refuses such a batch as well).

With IMQREF_TIME=1 it also times the two classes on 16 CPU threads over the benchmark's ROIs (bench.py's tile batch) and prints the
seconds.

The reference's Python package is not built here, so api_expected.json holds driver-recorded tables with the reference's user-facing
column names, passed through the table writer's "not finite -> soft_nan".
"""
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
from tests import imq_cases, imq_ref, parity  # noqa: E402


def build():
    ref = os.environ.get("REF", "/root/reference/src/nyx")
    w = tempfile.mkdtemp(prefix="imqref_")
    inc = ["-I/opt/conda/include"]
    for unit in ("focus_score", "saturation"):
        subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-w"] + inc + ["-c", f"{ref}/features/{unit}.cpp", "-o", f"{w}/{unit}.o"], check=True)
    objs = glob.glob(os.path.join(ROOT, "oracle", "_ref", "obj", "**", "*.o"), recursive=True)
    so = f"{w}/libimqref.so"
    subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-w", f"-I{ref}", f"-I{ROOT}/include"] + inc + ["-o", so,
                    os.path.join(HERE, "ref_imq_driver.cpp"), f"{w}/focus_score.o", f"{w}/saturation.o"] + objs +
                   ["/usr/lib/x86_64-linux-gnu/libtiff.so.5", "-lpthread"], check=True)
    lib = C.CDLL(so)
    lib.imqref_batch.restype = C.c_int
    lib.imqref_batch.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, s, n_threads=1, timed=False):
    assert int(b.bbox_w.min()) >= 2 and int(b.bbox_h.min()) >= 2, "a box with a side of 1 must never reach the reference (its loop does not end)"
    cb = b.c_struct()
    out = np.zeros((b.n_roi, 4))
    sec = np.zeros(1)
    rc = lib.imqref_batch(C.byref(cb), float(s.soft_nan), n_threads, out.ctypes.data, sec.ctypes.data if timed else None)
    assert rc == 0, rc
    return out, sec


def check(name, b, s, T):
    R = imq_ref.table(b, s)
    ok = imq_ref.same_bits(R[:, imq_ref.SATURATION], T[:, imq_ref.SATURATION])
    assert ok.all(), (name, "saturation", np.argwhere(~ok)[:8].tolist())
    rel = imq_ref.rel_diff(R[:, imq_ref.FOCUS], T[:, imq_ref.FOCUS])
    assert (rel <= parity.REL_TOL).all(), (name, "focus", float(rel.max()))
    return float(rel.max())


def main():
    lib = build()
    s = imq_cases.settings()
    store = {}
    worst = 0.0
    for name in imq_cases.CASES:
        b = imq_cases.batch(name)
        T, _ = ref_rows(lib, b, s)
        worst = max(worst, check(name, b, s, T))
        store[f"{name}__table"] = T
        print(f"{name}: {b.n_roi} ROIs, {int((~np.isfinite(T)).sum())} non-finite, {int((T == 0).sum())} zeros")
    pub = imq_cases.published()
    for c, col in enumerate(imq_cases.NAMES):
        got, want = store["published__table"][0, c], pub["expected"][col]
        assert abs(got - want) <= pub["rel_tol"] * abs(want), (col, got, want)
    # named properties of the cases
    assert (store["zeros__table"][0] == [0.0, 0.0, 1.0, 0.0]).all(), store["zeros__table"]
    assert (store["flat__table"][0, 2:] == [1.0, 0.0]).all(), store["flat__table"]
    # the API fixture: the ROIs of two tiles in (tile, label) order, and the two tiles as whole slides
    tb = imq_cases.tile_batch()
    T, _ = ref_rows(lib, tb, s)
    worst = max(worst, check("tile", tb, s, T))
    store["tile__table"] = T
    inten, lab = imq_cases.api_tiles()
    sb = imq_cases.slide_batch(inten)
    S, _ = ref_rows(lib, sb, s)
    worst = max(worst, check("slides", sb, s, S))
    store["slides__table"] = S
    np.savez_compressed(os.path.join(HERE, "imq_reference.npz"), **store)
    fin = lambda A: np.where(np.isfinite(A), A, s.soft_nan)
    N = imq_cases.NAMES
    pick = ["MIN_SATURATION", "FOCUS_SCORE"]
    order = sorted(pick, key=N.index)
    tiles = [t for t in range(lab.shape[0]) for _ in sorted(int(u) for u in np.unique(lab[t]) if u)]
    api = {"inten_dtype": "uint16", "labels": [int(v) for v in tb.roi_label], "tiles": tiles,
           "cases": {"two_codes": {"features": pick, "columns": order, "numeric": fin(T)[:, [N.index(c) for c in order]].tolist()},
                     "all_imq": {"features": ["*all_imq*"], "columns": list(N), "numeric": fin(T).tolist()}},
           "single_roi": {"features": ["*ALL_IMQ*"], "columns": list(N), "numeric": fin(S).tolist()}}
    json.dump(api, open(os.path.join(HERE, "api_expected.json"), "w"))
    print(f"largest relative difference restatement vs recording on the two focus columns: {worst:.3e}")
    if os.environ.get("IMQREF_TIME"):
        from tests import synth
        bb = synth.tile_batch(0)
        keep = (bb.bbox_w >= 2) & (bb.bbox_h >= 2)
        assert keep.all(), "the benchmark's tile batch holds a box with a side of 1"
        sec = min(ref_rows(lib, bb, s, n_threads=16, timed=True)[1][0] for _ in range(3))
        print(f"reference FocusScoreFeature + SaturationFeature, 16 threads, {bb.n_roi} ROIs of the benchmark tile: {sec * 1e3:.2f} ms = "
              f"{sec * 1e9 / bb.n_roi:.0f} ns per ROI")


if __name__ == "__main__":
    main()
