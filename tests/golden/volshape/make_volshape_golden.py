#!/usr/bin/env python3
"""Generates tests/golden/volshape/volshape_reference.npz and api_expected.json: the output of the reference's own D3_SurfaceFeature on the
inputs of tests/volshape_cases.py.  Only DATA is stored (per case the table [n_roi x 14]); the inputs are rebuilt from seeds.

The reference class is compiled OUTSIDE the repository, into a temporary directory: ref_volshape_driver.cpp (own code, next to this file)
and features/3d_surface.cpp of the reference where it lies, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    python tests/golden/volshape/make_volshape_golden.py    # REF=<reference>/src/nyx overrides the place of the reference sources

The driver is handed box-relative coordinates.  THE RULING: this package serves the exact hull volume, and the
reference's float quickhull is not exact.  For every ROI of volshape_cases.CASES the script asserts that the reference's hull volume
equals tests/volshape_ref.py's exact one within volshape_cases.HULL_AGREE -- a case that fails is replaced, nothing is excluded -- and
that the restatement agrees on every other column by the rules of volshape_cases (the eigen columns of a rank-deficient cloud are pinned
to the restatement's 0, decided from the inputs alone).  The clouds of volshape_cases.INEXACT are recorded under
"<case>__reference_inexact" as [reference hull volume, exact hull volume]: they document the ruling and are not compared.

It also prints, over a seeded sweep of random clouds, the largest relative hull difference among the ROIs that agree and the smallest
among those that do not: HULL_AGREE must lie orders of magnitude from both.  Coordinates stay small: the reference's quickhull aborts on
a ball near 60000, and nothing here comes near.

With VOLSHAPEREF_TIME=1 it also times the class on 16 CPU threads over the workloads of tools/vol_probe.py.

The reference's Python package is not built here, so api_expected.json holds driver-recorded values under the reference's user-facing
names as its table writer would show them ("not finite -> soft_nan"), with the hull columns asserted exact like every recorded ROI's.
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
from tests import vol_cases, volshape_cases, volshape_edge_cases, volshape_ref  # noqa: E402

UNITS = ("3d_surface",)
R = volshape_ref


def build():
    ref = os.environ.get("REF", "/root/reference/src/nyx")
    w = tempfile.mkdtemp(prefix="volshaperef_")
    inc = ["-I/opt/conda/include"]
    for unit in UNITS:
        subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-w"] + inc + ["-c", f"{ref}/features/{unit}.cpp", "-o", f"{w}/{unit}.o"], check=True)
    objs = [o for o in glob.glob(os.path.join(ROOT, "oracle", "_ref", "obj", "**", "*.o"), recursive=True) if os.path.basename(o)[:-2] not in UNITS]
    so = f"{w}/libvolshaperef.so"
    subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-w", f"-I{ref}", f"-I{ROOT}/include"] + inc + ["-o", so,
                    os.path.join(HERE, "ref_volshape_driver.cpp"), *[f"{w}/{u}.o" for u in UNITS]] + objs +
                   ["/usr/lib/x86_64-linux-gnu/libtiff.so.5", "-lpthread"], check=True)
    lib = C.CDLL(so)
    lib.volshaperef_batch.restype = C.c_int
    lib.volshaperef_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def ref_rows(lib, b, s, n_threads=1):
    assert int(max(b.bbox_w.max(), b.bbox_h.max(), b.bbox_d.max())) < 4096, "the reference's quickhull is kept away from large coordinates"
    cb = b.c_struct()
    out = np.zeros((b.n_roi, volshape_cases.N_COL))
    sec = np.zeros(1)
    rc = lib.volshaperef_batch(C.byref(cb), C.byref(s), n_threads, out.ctypes.data, sec.ctypes.data)
    assert rc == 0, rc
    return out, sec


def record(lib, b, s, label):
    """The recording of one case: the driver's table, with the exact hull and the restatement asserted on all of it."""
    T, _ = ref_rows(lib, b, s)
    W = R.table(b, s)
    fig = volshape_cases.figures(W, T, volshape_cases.eigen_compared(b))
    print(f"{label}: {b.n_roi} ROIs; restatement vs reference: hull {fig['hull']:.3e}, closed forms {fig['closed']:.3e}, eigen squares {fig['lens']:.3e}, "
          f"squared ratios {fig['ratios']:.3e}")
    assert (W[:, R.COL["3AREA"]] == T[:, R.COL["3AREA"]]).all(), label
    assert fig["hull"] <= volshape_cases.HULL_AGREE, (label, "the reference's hull is not exact here: replace the case", T[:, R.HULL[0]], W[:, R.HULL[0]])
    assert fig["closed"] <= volshape_cases.TOL_RESTATED and fig["lens"] <= volshape_cases.TOL and fig["ratios"] <= volshape_cases.TOL, (label, fig)
    return T


def sweep(lib, s):
    """random clouds: the relative hull difference reference / exact, split at HULL_AGREE"""
    rng = np.random.default_rng(2024)
    agree, differ = [], []
    for lo, hi, dens in ((2, 6, 0.5), (3, 10, 0.9), (3, 10, 0.5), (8, 20, 0.3)):
        rois = []
        while len(rois) < 60:
            d, h, w = rng.integers(lo, hi, 3)
            m = rng.random((d, h, w)) < dens
            if m.sum() >= 4:
                rois.append(volshape_edge_cases.from_mask(m))
        b = _abi.batch3d_from_rois(rois)
        T, _ = ref_rows(lib, b, s)
        exact = R.hull6_of(b) / 6.0
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(exact == T[:, R.HULL[0]], 0.0, np.abs(T[:, R.HULL[0]] - exact) / np.abs(exact))
        ok = rel <= volshape_cases.HULL_AGREE
        print(f"sweep: box sides {lo}..{hi - 1}, density {dens}: {int(ok.sum())} of {len(ok)} agree with the exact value")
        agree += list(rel[ok]); differ += list(rel[~ok])
    print(f"sweep: largest relative difference among agreeing ROIs {max(agree):.3e}, smallest among disagreeing ROIs {min(differ):.3e}; "
          f"HULL_AGREE = {volshape_cases.HULL_AGREE:.0e}")
    assert max(agree) * 1e3 < volshape_cases.HULL_AGREE < min(differ) * 1e-3


def main():
    lib = build()
    s = volshape_cases.settings()
    store = {}
    for name in volshape_cases.CASES:
        store[name] = record(lib, volshape_cases.batch(name), s, name)
    for name in volshape_cases.INEXACT:
        b = volshape_cases.batch(name)
        T, _ = ref_rows(lib, b, s)
        exact = R.hull6_of(b) / 6.0
        store[name + "__reference_inexact"] = np.stack([T[:, R.HULL[0]], exact], axis=1)
        print(f"{name}: reference hull volume {T[0, R.HULL[0]]:.4f}, exact {exact[0]:.4f} (recorded side by side, not compared)")
    np.savez_compressed(os.path.join(HERE, "volshape_reference.npz"), **store)
    sweep(lib, s)
    # the API fixture: the volumes of vol_cases.api_volumes(); expected = the recordings of their clouds under the user-facing names
    from nyxus_amd.nyxus3d import clouds_from_volume
    I, M = vol_cases.api_volumes()
    rois = [r for v in range(I.shape[0]) for r in clouds_from_volume(I[v].astype(np.uint32), M[v])]
    vols = [v for v in range(I.shape[0]) for _ in clouds_from_volume(I[v], M[v])]
    b = _abi.batch3d_from_rois(rois)
    Z = record(lib, b, s, "api")
    fin = np.where(np.isfinite(Z), Z, s.soft_nan)
    zone = json.load(open(os.path.join(os.path.dirname(HERE), "volzone", "api_expected.json")))
    json.dump({"labels": [int(v) for v in b.roi_label], "volumes": vols, "features": ["*3D_ALL_MORPHOLOGY*"], "coarse_gray_depth": 64,
               "metaparams": zone["metaparams"], "columns": featureset3d.SHAPE_3D, "numeric": fin.tolist()}, open(os.path.join(HERE, "api_expected.json"), "w"))
    if os.environ.get("VOLSHAPEREF_TIME"):                 # a child process per workload: the reference's quickhull may abort on one
        for wname in _workloads().WORKLOADS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--time", wname], capture_output=True, text=True)
            print(p.stdout.strip() if p.returncode == 0 else f"reference, 16 threads, {wname}: the class does not complete (exit status {p.returncode})")


def _workloads():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import vol_probe
    return vol_probe


def time_workload(wname):
    lib = build()
    bb = _workloads().workload(wname)
    sec = np.min([ref_rows(lib, bb, volshape_cases.settings(), n_threads=16)[1] for _ in range(2)], axis=0)
    print(f"reference, 16 threads, {wname}: shape class {sec[0] * 1e3:.1f} ms")


if __name__ == "__main__":
    time_workload(sys.argv[2]) if sys.argv[1:2] == ["--time"] else main()
