#!/usr/bin/env python3
"""Generates tests/golden/vol/vol_reference.npz and api_expected.json: the output of the reference's own D3_VoxelIntensityFeatures and
D3_GLCM_feature on the inputs of tests/vol_cases.py.  Only DATA is stored (per case the table [n_roi x 455]: 36 intensity codes, 30
angled GLCM codes x 13 directions, 29 _AVE codes); the inputs are rebuilt from seeds by tests/vol_cases.py.

The reference classes are compiled OUTSIDE the repository, into a temporary directory: ref_vol_driver.cpp (own code, next to this file)
and features/3d_intensity.cpp, features/3d_glcm.cpp, features/3d_glcm_nontriv.cpp of the reference where they lie, linked with the objects oracle/Makefile leaves in
oracle/_ref/obj:

    python tests/golden/vol/make_vol_golden.py          # REF=<reference>/src/nyx overrides the place of the reference sources

    g++ -std=c++20 -O2 -fPIC -w -I/opt/conda/include -c $REF/features/3d_intensity.cpp -o $W/3d_intensity.o      (and 3d_glcm.cpp, 3d_glcm_nontriv.cpp)
    g++ -std=c++20 -O2 -fPIC -shared -w -I$REF -Iinclude -I/opt/conda/include -o $W/libvolref.so tests/golden/vol/ref_vol_driver.cpp
        $W/3d_intensity.o $W/3d_glcm.o $W/3d_glcm_nontriv.o oracle/_ref/obj/**/*.o /usr/lib/x86_64-linux-gnu/libtiff.so.5 -lpthread

Before anything is stored, tests/vol_ref.py must agree with the driver on every value of every case -- integer-valued and
order-statistic columns bit for bit, the rest within parity.REL_TOL (vol_cases.compare) -- except where vol_cases.rule_excluded says the
reference is undefined: there the recording takes this package's defined value, by that rule and never by looking at a mismatch.  The
driver also reports which _AVE codes save_value assigns (all 29).

With VOLREF_TIME=1 it also times the two classes on 16 CPU threads over the workloads of tools/vol_probe.py and prints the seconds.

The reference's Python package is not built here, so api_expected.json holds driver-recorded values under the reference's user-facing
names as its table writer would show them: one value per code (fvals[code][0]: direction shifts[0] of an angled code), "not finite ->
soft_nan".
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
from tests import vol_cases, vol_ref  # noqa: E402


UNITS = ("3d_intensity", "3d_glcm", "3d_glcm_nontriv")     # (the last one holds the out-of-core methods the class declares)


def build():
    ref = os.environ.get("REF", "/root/reference/src/nyx")
    w = tempfile.mkdtemp(prefix="volref_")
    inc = ["-I/opt/conda/include"]
    for unit in UNITS:
        subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-w"] + inc + ["-c", f"{ref}/features/{unit}.cpp", "-o", f"{w}/{unit}.o"], check=True)
    objs = [o for o in glob.glob(os.path.join(ROOT, "oracle", "_ref", "obj", "**", "*.o"), recursive=True)
            if os.path.basename(o)[:-2] not in UNITS]
    so = f"{w}/libvolref.so"
    subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-w", f"-I{ref}", f"-I{ROOT}/include"] + inc + ["-o", so,
                    os.path.join(HERE, "ref_vol_driver.cpp"), *[f"{w}/{u}.o" for u in UNITS]] + objs +
                   ["/usr/lib/x86_64-linux-gnu/libtiff.so.5", "-lpthread"], check=True)
    lib = C.CDLL(so)
    lib.volref_batch.restype = C.c_int
    lib.volref_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, s, n_threads=1, timed=False):
    cb = b.c_struct()
    out = np.zeros((b.n_roi, vol_cases.N_COL))
    assigned = np.zeros(vol_cases.N_AVE, np.int32)
    sec = np.zeros(1)
    rc = lib.volref_batch(C.byref(cb), C.byref(s), n_threads, out.ctypes.data, assigned.ctypes.data, sec.ctypes.data if timed else None)
    assert rc == 0, rc
    return out, assigned, sec


def record(lib, b, s, label):
    """The recording of one case: the driver's table with the rule-excluded values replaced by the defined ones; vol_ref asserted on the
    rest.  Returns (table, largest relative differences of the two blocks)."""
    T, assigned, _ = ref_rows(lib, b, s)
    assert assigned.all(), (label, "save_value left an _AVE code unassigned", assigned.tolist())
    R = vol_ref.table(b, s)
    ex = vol_cases.rule_excluded(b, s)
    T = np.where(ex, R, T)
    bad, ri, rg = vol_cases.compare(R, T)
    assert not bad, (label, bad[:10])
    return T, ri, rg


def main():
    lib = build()
    store, wi, wg = {}, 0.0, 0.0
    for bname, mode in vol_cases.CASES:
        b, s = vol_cases.batch(bname), vol_cases.settings(mode)
        T, ri, rg = record(lib, b, s, (bname, mode))
        wi, wg = max(wi, ri), max(wg, rg)
        store[vol_cases.case_name(bname, mode)] = T
        print(f"{bname} / {mode}: {b.n_roi} ROIs, {int((~np.isfinite(T)).sum())} non-finite, {int(vol_cases.rule_excluded(b, s).sum())} values by rule; "
              f"restatement vs reference: intensity {ri:.3e}, GLCM {rg:.3e}")
    np.savez_compressed(os.path.join(HERE, "vol_reference.npz"), **store)
    print(f"largest relative difference restatement vs recording: intensity block {wi:.3e}, GLCM block {wg:.3e}")
    # the API fixture: two volumes with labelled ROIs; expected = the recording of their clouds under the user-facing names
    from nyxus_amd.nyxus3d import clouds_from_volume
    I, M = vol_cases.api_volumes()
    rois = [r for v in range(I.shape[0]) for r in clouds_from_volume(I[v], M[v])]
    vols = [v for v in range(I.shape[0]) for _ in clouds_from_volume(I[v], M[v])]
    b = _abi.batch3d_from_rois(rois)
    s = _abi.default_settings(64)
    s.glcm_grey_depth = 64
    T, _, _ = record(lib, b, s, "api")
    names = vol_cases.column_names()
    fin = np.where(np.isfinite(T), T, s.soft_nan)
    cases = {}
    for key, feats in (("groups", ["*3D_ALL_INTENSITY*", "*3D_GLCM*"]), ("codes", ["3GLCM_CONTRAST_AVE", "3MEAN", "3GLCM_ACOR", "3P99"])):
        _, req = featureset3d.expand3d(feats)
        cases[key] = {"features": feats, "columns": req, "numeric": fin[:, [names.index(featureset3d.table_column(c)) for c in req]].tolist()}
    json.dump({"labels": [int(v) for v in b.roi_label], "volumes": vols, "cases": cases}, open(os.path.join(HERE, "api_expected.json"), "w"))
    if os.environ.get("VOLREF_TIME"):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import vol_probe
        for wname in vol_probe.WORKLOADS:
            for gd in (64, vol_cases.LEVEL_CAP):
                bb = vol_probe.workload(wname)
                ss = _abi.default_settings(64)
                ss.glcm_grey_depth = gd
                sec = min(ref_rows(lib, bb, ss, n_threads=16, timed=True)[2][0] for _ in range(2))
                nvox = int(bb.px_offset[-1])
                print(f"reference D3_VoxelIntensityFeatures + D3_GLCM_feature, 16 threads, {wname}, grey depth {gd}: {sec * 1e3:.1f} ms = {sec * 1e9 / nvox:.1f} ns per voxel")


if __name__ == "__main__":
    main()
