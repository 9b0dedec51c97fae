#!/usr/bin/env python3
"""Generates tests/golden/volzone/volzone_reference.npz and api_expected.json: the output of the reference's own D3_GLRLM_feature and
D3_GLSZM_feature on the inputs of tests/volzone_cases.py.  Only DATA is stored (per case the table [n_roi x 240]); the inputs are rebuilt
from seeds.

The reference classes are compiled OUTSIDE the repository, into a temporary directory: ref_volzone_driver.cpp (own code, next to this
file) and features/3d_glrlm.cpp, 3d_glrlm_nontriv.cpp, 3d_glszm.cpp of the reference where they lie, linked with the objects
oracle/Makefile leaves in oracle/_ref/obj:

    python tests/golden/volzone/make_volzone_golden.py    # REF=<reference>/src/nyx overrides the place of the reference sources

Before anything is stored, tests/volzone_ref.py must agree with the driver on every value of every case within parity.REL_TOL
(volzone_cases.compare) -- except where volzone_cases.rule_excluded says the reference is undefined: there the recording takes this
package's defined value, by that rule and never by looking at a mismatch.  Every case asserts that the rule takes out at most 5 % of its
values, and none in an ROI the rule does not name.

With VOLZONEREF_TIME=1 it also times the two classes on 16 CPU threads over the workloads of tools/vol_probe.py.

The reference's Python package is not built here, so api_expected.json holds driver-recorded values under the reference's user-facing
names as its table writer would show them ("not finite -> soft_nan"; an angled code shows direction 0).
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
from tests import volzone_cases, volzone_ref  # noqa: E402

UNITS = ("3d_glrlm", "3d_glrlm_nontriv", "3d_glszm")


def build():
    ref = os.environ.get("REF", "/root/reference/src/nyx")
    w = tempfile.mkdtemp(prefix="volzoneref_")
    inc = ["-I/opt/conda/include"]
    for unit in UNITS:
        subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-w"] + inc + ["-c", f"{ref}/features/{unit}.cpp", "-o", f"{w}/{unit}.o"], check=True)
    objs = [o for o in glob.glob(os.path.join(ROOT, "oracle", "_ref", "obj", "**", "*.o"), recursive=True) if os.path.basename(o)[:-2] not in UNITS]
    so = f"{w}/libvolzoneref.so"
    subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-w", f"-I{ref}", f"-I{ROOT}/include"] + inc + ["-o", so,
                    os.path.join(HERE, "ref_volzone_driver.cpp"), *[f"{w}/{u}.o" for u in UNITS]] + objs +
                   ["/usr/lib/x86_64-linux-gnu/libtiff.so.5", "-lpthread"], check=True)
    lib = C.CDLL(so)
    lib.volzoneref_batch.restype = C.c_int
    lib.volzoneref_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, s, t, n_threads=1):
    cb = b.c_struct()
    out = np.zeros((b.n_roi, volzone_cases.N_COL))
    sec = np.zeros(2)
    rc = lib.volzoneref_batch(C.byref(cb), C.byref(s), C.byref(t), n_threads, out.ctypes.data, sec.ctypes.data)
    assert rc == 0, rc
    return out, sec


def record(lib, b, s, t, label):
    """The recording of one case: the driver's table with the rule-excluded values replaced by the defined ones; volzone_ref asserted on
    the rest.  Returns (table, largest relative difference)."""
    T, _ = ref_rows(lib, b, s, t)
    R = volzone_ref.table(b, s, t)
    ex = volzone_cases.rule_excluded(b, s, t)
    T = np.where(ex, R, T)
    bad, rel = volzone_cases.compare(R, T)
    assert not bad, (label, bad[:10])
    return T, rel


def main():
    lib = build()
    store, worst = {}, 0.0
    for bname, mode in volzone_cases.CASES:
        b = volzone_cases.batch(bname)
        s, t = volzone_cases.settings(mode)
        T, rel = record(lib, b, s, t, (bname, mode))
        worst = max(worst, rel)
        store[volzone_cases.case_name(bname, mode)] = T
        ex = volzone_cases.rule_excluded(b, s, t)
        named = np.zeros(b.n_roi, bool)
        named[:2] = bname == "rule"                        # the two ROIs that batch was built to hold (volzone_cases._rule)
        assert ex.mean() <= 0.05 and not ex[~named].any(), (bname, mode, ex.mean())
        print(f"{bname} / {mode}: {b.n_roi} ROIs, {int((~np.isfinite(T)).sum())} non-finite, {int(ex.sum())} values by rule ({100 * ex.mean():.1f} %); "
              f"restatement vs reference {rel:.3e}")
    np.savez_compressed(os.path.join(HERE, "volzone_reference.npz"), **store)
    print(f"largest relative difference restatement vs recording: {worst:.3e}")
    # the API fixture: the volumes of vol_cases.api_volumes(); expected = the recordings of their clouds under the user-facing names
    from nyxus_amd.nyxus3d import clouds_from_volume
    I, M = volzone_cases.api_volumes()
    rois = [r for v in range(I.shape[0]) for r in clouds_from_volume(I[v], M[v])]
    vols = [v for v in range(I.shape[0]) for _ in clouds_from_volume(I[v], M[v])]
    b = _abi.batch3d_from_rois(rois)
    s = _abi.default_settings(64)
    zt = _abi.VolZoneSettings(0, 0)
    fields = {"3glrlm/greydepth": "glrlm_grey_depth", "3glszm/greydepth": "glszm_grey_depth"}
    for m in volzone_cases.API_METAPARAMS:
        k, v = m.split("=")
        if k in fields:                                    # (the others belong to the classes Nyxus3D serves: tests/golden/voltex)
            setattr(zt, fields[k], int(v))
    Z, _ = ref_rows(lib, b, s, zt)
    R = volzone_ref.table(b, s, zt)
    Z = np.where(volzone_cases.rule_excluded(b, s, zt), R, Z)
    bad, _ = volzone_cases.compare(R, Z)
    assert not bad, bad[:10]
    names = volzone_cases.column_names()
    full = Z
    feats = ["*3D_GLRLM*", "*3D_GLSZM*"]
    _, req = featureset3d.expand3d_zones(feats)
    sel = [names.index(featureset3d.table_column(c)) for c in req]
    fin = np.where(np.isfinite(full), full, s.soft_nan)
    json.dump({"labels": [int(v) for v in b.roi_label], "volumes": vols, "features": feats, "metaparams": volzone_cases.API_METAPARAMS, "columns": req,
               "numeric": fin[:, sel].tolist()}, open(os.path.join(HERE, "api_expected.json"), "w"))
    if os.environ.get("VOLZONEREF_TIME"):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import vol_probe
        for wname in vol_probe.WORKLOADS:
            bb = vol_probe.workload(wname)
            ss = _abi.default_settings(64)
            sec = np.min([ref_rows(lib, bb, ss, _abi.VolZoneSettings(64, 64), n_threads=16)[1] for _ in range(2)], axis=0)
            print(f"reference, 16 threads, {wname}, grey depth 64: GLRLM {sec[0] * 1e3:.1f} ms, GLSZM {sec[1] * 1e3:.1f} ms")


if __name__ == "__main__":
    main()
