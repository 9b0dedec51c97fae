#!/usr/bin/env python3
"""Generates tests/golden/ih/ih_reference.npz and api_expected.json: the output of the reference's own IntensityHistogramFeatures on the
inputs of tests/ih_cases.py.  Only DATA is stored (per ROI the 46 values as the class leaves them, NaN / inf included, and the N bin
counts); the inputs are rebuilt from seeds by tests/ih_cases.py.  published.json (the two tables the reference's tests carry) is not
generated: it is transcribed.

The reference class is compiled OUTSIDE the repository, into a temporary directory: ref_ih_driver.cpp (own code, next to this file) and
features/intensity_histogram.cpp of the reference where it lies, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    python tests/golden/ih/make_ih_golden.py            # REF=<reference>/src/nyx overrides the place of the reference sources

Before anything is stored, tests/ih_ref.py must equal the recording bit for bit on ih_ref.EXACT (NaN where the recording has NaN) and within
parity.REL_TOL on the two entropy columns (numpy's / Python's log need not be glibc's), the recorded counts must equal ih_ref.counts, and
the two published tables must hold on the recording.

With IHREF_TIME=1 it also times the class on 16 CPU threads over the benchmark's ROIs (bench.py's tile batch) and over a heavy-tailed
batch, and prints the seconds.

The reference's Python package is not built here, so api_expected.json holds driver-recorded tables with the reference's user-facing
column names (featureset.cpp UserFacingFeatureNames), passed through the table writer's "not finite -> soft_nan".
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
from tests import ih_cases, ih_ref, parity  # noqa: E402


def build():
    ref = os.environ.get("REF", "/root/reference/src/nyx")
    w = tempfile.mkdtemp(prefix="ihref_")
    inc = ["-I/opt/conda/include"]
    subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-w"] + inc + ["-c", f"{ref}/features/intensity_histogram.cpp", "-o", f"{w}/ih.o"], check=True)
    objs = glob.glob(os.path.join(ROOT, "oracle", "_ref", "obj", "**", "*.o"), recursive=True)
    so = f"{w}/libihref.so"
    subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-w", f"-I{ref}", f"-I{ROOT}/include"] + inc + ["-o", so,
                    os.path.join(HERE, "ref_ih_driver.cpp"), f"{w}/ih.o"] + objs + ["/usr/lib/x86_64-linux-gnu/libtiff.so.5", "-lpthread"], check=True)
    lib = C.CDLL(so)
    lib.ihref_batch.restype = C.c_int
    lib.ihref_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, s, n_threads=1, timed=False):
    cb = b.c_struct()
    n, N = b.n_roi, int(s.grey_depth)
    out = np.zeros((n, 46))
    cnt = np.zeros((n, max(N, 0)), np.uint64)
    sec = np.zeros(1)
    rc = lib.ihref_batch(C.byref(cb), N, int(s.ibsi), float(s.soft_nan), n_threads, out.ctypes.data, cnt.ctypes.data if N >= 2 else None,
                         sec.ctypes.data if timed else None)
    assert rc == 0, rc
    return out, cnt, sec


def check_and_pack(name, b, s, T, cnt, store):
    R = ih_ref.table(b, s)
    ex = [ih_ref.NAMES.index(c) for c in ih_ref.EXACT]
    en = [ih_ref.NAMES.index(c) for c in ih_ref.ENTROPY]
    ok = ih_ref.same(R[:, ex], T[:, ex])
    assert ok.all(), (name, [(r, ih_ref.EXACT[c], R[r, ex[c]], T[r, ex[c]]) for r, c in np.argwhere(~ok)[:8]])
    a, w = R[:, en], T[:, en]
    rel = np.where(ih_ref.same(a, w), 0.0, np.abs(a - w) / np.maximum(np.abs(w), 1e-300))
    assert (rel <= parity.REL_TOL).all(), (name, rel.max())
    N = int(s.grey_depth)
    flat, off = [], [0]
    for r in range(b.n_roi):
        o, e = int(b.px_offset[r]), int(b.px_offset[r + 1])
        gated = not s.ibsi or N < 2 or b.max_inten[r] <= b.min_inten[r]
        if gated:
            assert (T[r] == s.soft_nan).all(), (name, r)
            off.append(off[-1])
            continue
        want = ih_ref.counts(b.inten[o:e], int(b.min_inten[r]), int(b.max_inten[r]), N)
        assert (want == cnt[r].astype(np.int64)).all() and int(cnt[r].sum()) == e - o, (name, r)
        flat.append(cnt[r].astype(np.uint32) if cnt[r].max() < 2 ** 32 else cnt[r])
        off.append(off[-1] + N)
    store[f"{name}__table"] = T
    store[f"{name}__counts"] = np.concatenate(flat).astype(np.uint32) if flat else np.zeros(0, np.uint32)
    store[f"{name}__counts_offset"] = np.asarray(off, np.int64)
    return float(rel.max())


def main():
    lib = build()
    store = {}
    worst = 0.0
    for name in ih_cases.CASES:
        b, s = ih_cases.batch(name), ih_cases.settings(name)
        T, cnt, _ = ref_rows(lib, b, s)
        worst = max(worst, check_and_pack(name, b, s, T, cnt, store))
        print(f"{name}: {b.n_roi} ROIs, N = {s.grey_depth}, {int(np.isnan(T).sum())} NaN, {int(np.isinf(T).sum())} inf, "
              f"{int((T == s.soft_nan).all(axis=1).sum())} gated rows")
    # the published tables hold on the recording
    pub = ih_cases.published()
    for key, case in (("five_pixel", "five"), ("ibsi_phantom", "phantom")):
        row = store[f"{case}__table"][0]
        for col, want in pub[key]["expected"].items():
            got = row[ih_ref.NAMES.index(col)]
            assert abs(got - want) <= pub[key]["rel_tol"] * abs(want) + (1e-9 if want == 0 else 0.0), (key, col, got, want)
    # named properties of the cases
    assert store["flat_big__counts"].max() > 65535
    g = ih_ref.NAMES.index("IH_MAX_GRADIENT")
    assert (store["no_gradient__table"][:2, g] == ih_ref.DBL_MIN).all() and (store["no_gradient__table"][:2, g + 1] == 0).all()
    assert store["no_gradient__table"][2, g] == 1.0 and store["no_gradient__table"][2, g + 1] == 1.0
    assert (store["gate_negative_depth__table"] == ih_cases.SOFT_NAN).all() and (store["gate_ibsi_off__table"] == ih_cases.SOFT_NAN).all()
    assert (store["gates__table"] == ih_cases.SOFT_NAN).all()
    # the API fixture: one tile, rows in label order
    tb = ih_cases.tile_batch()
    s = ih_cases.settings("sizes")
    s.grey_depth = ih_cases.API_DEPTH
    T, cnt, _ = ref_rows(lib, tb, s)
    worst = max(worst, check_and_pack("tile", tb, s, T, cnt, store))
    np.savez_compressed(os.path.join(HERE, "ih_reference.npz"), **store)
    F = np.where(np.isfinite(T), T, s.soft_nan)
    N = ih_ref.NAMES
    pick = ["IH_BIN_SIZE", "IH_MEAN_VAL", "IH_P90_IDX"]
    order = sorted(pick, key=N.index)
    api = {"inten_dtype": "uint16", "coarse_gray_depth": ih_cases.API_DEPTH, "labels": [int(v) for v in tb.roi_label],
           "cases": {"three_codes": {"features": pick, "columns": order, "numeric": F[:, [N.index(c) for c in order]].tolist()},
                     "all_ih": {"features": ["*ALL_IH*"], "columns": list(N), "numeric": F.tolist()}}}
    json.dump(api, open(os.path.join(HERE, "api_expected.json"), "w"))
    print(f"largest relative difference restatement vs recording on the entropy columns: {worst:.3e}")
    if os.environ.get("IHREF_TIME"):
        from tests import radial_cases, synth
        from nyxus_amd import _abi
        s = _abi.default_settings(64, True)
        for tag, bb in (("the benchmark tile", synth.tile_batch(0)), ("the heavy-tailed batch", _abi.batch_from_rois(radial_cases.heavy()))):
            sec = min(ref_rows(lib, bb, s, n_threads=16, timed=True)[2][0] for _ in range(3))
            print(f"reference IntensityHistogramFeatures, 16 threads, {bb.n_roi} ROIs of {tag}: {sec * 1e3:.2f} ms = {sec * 1e9 / bb.n_roi:.0f} ns per ROI")


if __name__ == "__main__":
    main()
