#!/usr/bin/env python3
"""Generates tests/golden/voldzone/voldzone_reference.npz and api_expected.json: the output of the reference's own D3_GLDZM_feature on the
inputs of tests/voldzone_cases.py.  Only DATA is stored (per case the table [n_roi x 18]); the inputs are rebuilt from seeds.

The reference class is compiled OUTSIDE the repository, into a temporary directory: ref_voldzone_driver.cpp (own code, next to this file)
and features/3d_gldzm.cpp of the reference where it lies, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    python tests/golden/voldzone/make_voldzone_golden.py    # REF=<reference>/src/nyx overrides the place of the reference sources

THE DRIVER IS NEVER HANDED A RULE-EXCLUDED ROI (voldzone_cases.rule_excluded): outside IBSI mode the reference writes
outside its matrix for a box that holds a level-0 cell.  Every case of voldzone_cases.CASES must contain no such ROI -- asserted before
the driver is called -- and before anything is stored tests/voldzone_ref.py must agree with the driver on every value within
parity.REL_TOL, with NaN / inf in the same places.  The cases of voldzone_cases.RULE_CASES are recorded from the restatement alone, under
the key "<case>__restated".

With VOLDZONEREF_TIME=1 it also times the class on 16 CPU threads over the workloads of tools/vol_probe.py at grey depth 64 (matlab
binning: no level-0 cell, the reference is defined).

The reference's Python package is not built here, so api_expected.json holds driver-recorded values under the reference's user-facing
names as its table writer would show them ("not finite -> soft_nan").
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
from nyxus_amd import _abi, featureset3d  # noqa: E402
from tests import voldzone_cases, voldzone_ref  # noqa: E402

UNITS = ("3d_gldzm",)


def build():
    ref = os.environ.get("REF", "/root/reference/src/nyx")
    w = tempfile.mkdtemp(prefix="voldzoneref_")
    inc = ["-I/opt/conda/include"]
    for unit in UNITS:
        subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-w"] + inc + ["-c", f"{ref}/features/{unit}.cpp", "-o", f"{w}/{unit}.o"], check=True)
    objs = [o for o in glob.glob(os.path.join(ROOT, "oracle", "_ref", "obj", "**", "*.o"), recursive=True) if os.path.basename(o)[:-2] not in UNITS]
    so = f"{w}/libvoldzoneref.so"
    subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-w", f"-I{ref}", f"-I{ROOT}/include"] + inc + ["-o", so,
                    os.path.join(HERE, "ref_voldzone_driver.cpp"), *[f"{w}/{u}.o" for u in UNITS]] + objs +
                   ["/usr/lib/x86_64-linux-gnu/libtiff.so.5", "-lpthread"], check=True)
    lib = C.CDLL(so)
    lib.voldzoneref_batch.restype = C.c_int
    lib.voldzoneref_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, s, n_threads=1):
    assert not voldzone_cases.rule_excluded(b, s).any(), "the reference is never run on a rule-excluded ROI"
    cb = b.c_struct()
    out = np.zeros((b.n_roi, voldzone_cases.N_COL))
    sec = np.zeros(1)
    rc = lib.voldzoneref_batch(C.byref(cb), C.byref(s), n_threads, out.ctypes.data, sec.ctypes.data)
    assert rc == 0, rc
    return out, sec


def record(lib, b, s, label):
    """The recording of one case: the driver's table, with voldzone_ref asserted on all of it.  Returns (table, largest relative
    difference)."""
    T, _ = ref_rows(lib, b, s)
    R = voldzone_ref.table(b, s)
    assert (np.isnan(R) == np.isnan(T)).all() and (np.isinf(R) == np.isinf(T)).all(), label
    bad, rel = voldzone_cases.compare(R, T)
    assert not bad, (label, bad[:10])
    return T, rel


def main():
    lib = build()
    store, worst = {}, 0.0
    for bname, mode in voldzone_cases.CASES:
        b = voldzone_cases.batch(bname)
        s = voldzone_cases.settings(mode)
        T, rel = record(lib, b, s, (bname, mode))
        worst = max(worst, rel)
        store[voldzone_cases.case_name(bname, mode)] = T
        print(f"{bname} / {mode}: {b.n_roi} ROIs, {int((~np.isfinite(T)).sum())} non-finite; restatement vs reference {rel:.3e}")
    for bname, mode in voldzone_cases.RULE_CASES:          # the restatement alone: the reference's code is not run on these
        b = voldzone_cases.batch(bname)
        s = voldzone_cases.settings(mode)
        ex = voldzone_cases.rule_excluded(b, s)
        assert ex.any()
        store[voldzone_cases.case_name(bname, mode) + "__restated"] = voldzone_ref.table(b, s)
        print(f"{bname} / {mode}: {b.n_roi} ROIs, {int(ex.sum())} rule-excluded; recorded from the restatement")
    np.savez_compressed(os.path.join(HERE, "voldzone_reference.npz"), **store)
    print(f"largest relative difference restatement vs recording: {worst:.3e}")
    # the API fixture: the volumes of vol_cases.api_volumes(); expected = the recordings of their clouds under the user-facing names
    from nyxus_amd.nyxus3d import clouds_from_volume
    I, M = voldzone_cases.api_volumes()
    rois = [r for v in range(I.shape[0]) for r in clouds_from_volume(I[v], M[v])]
    vols = [v for v in range(I.shape[0]) for _ in clouds_from_volume(I[v], M[v])]
    b = _abi.batch3d_from_rois(rois)
    s = _abi.default_settings(64)
    Z, _ = record(lib, b, s, "api")
    feats = ["*3D_GLDZM*"]
    _, req = featureset3d.expand3d_dzones(feats)
    names = voldzone_cases.column_names()
    sel = [names.index(featureset3d.table_column(c)) for c in req]
    fin = np.where(np.isfinite(Z), Z, s.soft_nan)
    json.dump({"labels": [int(v) for v in b.roi_label], "volumes": vols, "features": feats, "coarse_gray_depth": 64, "columns": req,
               "numeric": fin[:, sel].tolist()}, open(os.path.join(HERE, "api_expected.json"), "w"))
    if os.environ.get("VOLDZONEREF_TIME"):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import vol_probe
        for wname in vol_probe.WORKLOADS:
            bb = vol_probe.workload(wname)
            ss = _abi.default_settings(64)
            sec = np.min([ref_rows(lib, bb, ss, n_threads=16)[1] for _ in range(2)], axis=0)
            print(f"reference, 16 threads, {wname}, grey depth 64: GLDZM {sec[0] * 1e3:.1f} ms")


if __name__ == "__main__":
    main()
