#!/usr/bin/env python3
"""Generates tests/golden/voltex/voltex_reference.npz and api_expected.json: the output of the reference's own D3_GLDM_feature,
D3_NGLDM_feature and D3_NGTDM_feature on the inputs of tests/voltex_cases.py.  Only DATA is stored (per case the table [n_roi x 38]);
the inputs are rebuilt from seeds.

The reference classes are compiled OUTSIDE the repository, into a temporary directory: ref_voltex_driver.cpp (own code, next to this
file) and features/3d_gldm.cpp, 3d_ngldm.cpp, 3d_ngtdm.cpp of the reference where they lie, linked with the objects oracle/Makefile
leaves in oracle/_ref/obj (3d_ngtdm.cpp defines a non-static global `nsh`; no other unit of the link defines one):

    python tests/golden/voltex/make_voltex_golden.py    # REF=<reference>/src/nyx overrides the place of the reference sources

Before anything is stored, tests/voltex_ref.py must agree with the driver on every value of every case within parity.REL_TOL
(voltex_cases.compare) -- except where voltex_cases.rule_excluded says the reference is undefined: there the recording takes this
package's defined value, by that rule and never by looking at a mismatch.

With VOLTEXREF_TIME=1 it also times the three classes on 16 CPU threads over the workloads of tools/vol_probe.py.

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
from tests import voltex_cases, voltex_ref  # noqa: E402

UNITS = ("3d_gldm", "3d_ngldm", "3d_ngtdm")


def build():
    ref = os.environ.get("REF", "/root/reference/src/nyx")
    w = tempfile.mkdtemp(prefix="voltexref_")
    inc = ["-I/opt/conda/include"]
    for unit in UNITS:
        subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-w"] + inc + ["-c", f"{ref}/features/{unit}.cpp", "-o", f"{w}/{unit}.o"], check=True)
    objs = [o for o in glob.glob(os.path.join(ROOT, "oracle", "_ref", "obj", "**", "*.o"), recursive=True) if os.path.basename(o)[:-2] not in UNITS]
    so = f"{w}/libvoltexref.so"
    subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-w", f"-I{ref}", f"-I{ROOT}/include"] + inc + ["-o", so,
                    os.path.join(HERE, "ref_voltex_driver.cpp"), *[f"{w}/{u}.o" for u in UNITS]] + objs +
                   ["/usr/lib/x86_64-linux-gnu/libtiff.so.5", "-lpthread"], check=True)
    lib = C.CDLL(so)
    lib.voltexref_batch.restype = C.c_int
    lib.voltexref_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, s, t, n_threads=1):
    cb = b.c_struct()
    out = np.zeros((b.n_roi, voltex_cases.N_COL))
    sec = np.zeros(3)
    rc = lib.voltexref_batch(C.byref(cb), C.byref(s), C.byref(t), n_threads, out.ctypes.data, sec.ctypes.data)
    assert rc == 0, rc
    return out, sec


def record(lib, b, s, t, label):
    """The recording of one case: the driver's table with the rule-excluded values replaced by the defined ones; voltex_ref asserted on
    the rest.  Returns (table, largest relative difference)."""
    T, _ = ref_rows(lib, b, s, t)
    R = voltex_ref.table(b, s, t)
    ex = voltex_cases.rule_excluded(b, s, t)
    T = np.where(ex, R, T)
    bad, rel = voltex_cases.compare(R, T)
    assert not bad, (label, bad[:10])
    return T, rel


def main():
    lib = build()
    store, worst = {}, 0.0
    for bname, mode in voltex_cases.CASES:
        b = voltex_cases.batch(bname)
        s, t = voltex_cases.settings(mode)
        T, rel = record(lib, b, s, t, (bname, mode))
        worst = max(worst, rel)
        store[voltex_cases.case_name(bname, mode)] = T
        ex = voltex_cases.rule_excluded(b, s, t)
        nonflat = (b.max_inten != b.min_inten) & (b.counts() > 0)
        assert ex.mean() <= 0.05 and not ex[nonflat].any(), (bname, mode, ex.mean())
        print(f"{bname} / {mode}: {b.n_roi} ROIs, {int((~np.isfinite(T)).sum())} non-finite, {int(ex.sum())} values by rule ({100 * ex.mean():.1f} %); "
              f"restatement vs reference {rel:.3e}")
    np.savez_compressed(os.path.join(HERE, "voltex_reference.npz"), **store)
    print(f"largest relative difference restatement vs recording: {worst:.3e}")
    # the API fixture: the volumes of vol_cases.api_volumes(); expected = the recording of their clouds under the user-facing names
    from nyxus_amd.nyxus3d import clouds_from_volume
    I, M = voltex_cases.api_volumes()
    rois = [r for v in range(I.shape[0]) for r in clouds_from_volume(I[v], M[v])]
    vols = [v for v in range(I.shape[0]) for _ in clouds_from_volume(I[v], M[v])]
    b = _abi.batch3d_from_rois(rois)
    s = _abi.default_settings(64)
    names = voltex_cases.column_names()
    cases = {}
    for key, feats, meta in (("set", ["*3D_GLDM*", "*3D_NGLDM*", "*3D_NGTDM*"], voltex_cases.API_METAPARAMS), ("defaults", ["*3D_NGLDM*", "*3D_NGTDM*"], [])):
        t = _abi.VolTexSettings(0, 0, 0)
        for m in meta:
            k, v = m.split("=")
            setattr(t, {"3gldm/greydepth": "gldm_grey_depth", "3ngtdm/greydepth": "ngtdm_grey_depth", "3ngtdm/radius": "ngtdm_radius"}[k], int(v))
        T, _ = ref_rows(lib, b, s, t)
        R = voltex_ref.table(b, s, t)
        T = np.where(voltex_cases.rule_excluded(b, s, t), R, T)
        _, req = featureset3d.expand3d(feats)
        sel = [names.index(c) for c in req]
        bad, _ = voltex_cases.compare(R[:, sel], T[:, sel], req)
        assert not bad, (key, bad[:10])
        fin = np.where(np.isfinite(T), T, s.soft_nan)
        cases[key] = {"features": feats, "metaparams": meta, "columns": req, "numeric": fin[:, sel].tolist()}
    json.dump({"labels": [int(v) for v in b.roi_label], "volumes": vols, "cases": cases}, open(os.path.join(HERE, "api_expected.json"), "w"))
    if os.environ.get("VOLTEXREF_TIME"):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import vol_probe
        for wname in vol_probe.WORKLOADS:
            bb = vol_probe.workload(wname)
            ss = _abi.default_settings(64)
            tt = _abi.VolTexSettings(64, 64, 1)
            sec = np.min([ref_rows(lib, bb, ss, tt, n_threads=16)[1] for _ in range(2)], axis=0)
            print(f"reference, 16 threads, {wname}, grey depth 64, radius 1: GLDM {sec[0] * 1e3:.1f} ms, NGLDM {sec[1] * 1e3:.1f} ms, NGTDM {sec[2] * 1e3:.1f} ms")


if __name__ == "__main__":
    main()
