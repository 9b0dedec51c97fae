#!/usr/bin/env python3
"""Cost of the device label scan for volumes (nyxhip_assemble_volumes) beside the host assembly it replaces, on the three workloads of
tools/vol_probe.py packed into label volumes -- 64 ROIs of ~32^3 in 128^3 ("r32"), 4 ROIs of ~128^3 in 256 x 256 x 128 ("r128"), 2000
ROIs of ~8^3 in 128 x 128 x 64 ("r8") -- and on one confetti volume of 110592 labels (2 x 2 x 2 blocks of shuffled 32-bit labels in 96^3,
"confetti").  uint16 intensities, uint32 labels.  Per workload, `--runs` alternating runs (default 5) in one process after a warm-up,
medians and ranges in ms, host to host:
  (a) host      clouds_from_volume + batch3d_from_rois, and the host-to-device copy of the batch's arrays that a volume entry implies
  (b) dev/host  nyxhip_assemble_volumes from host volumes (their copy included)
  (c) dev/dev   nyxhip_assemble_volumes from device volumes; its volume bytes per second as a share of the HBM rate bench.py uses for its
                roofline (the whole call: scan, sort, clouds and three read-backs)
  (d) e2e       Nyxus3DShape(["*3D_ALL*"]).featurize at grey depth 64, assembly="host" against assembly="device" (--e2e WORKLOADS; default all)
--launches also prints the time of every launch of the scan: this script once more per workload as a child process under
`rocprofv3 --kernel-trace --stats` (a trace on its own, no counters beside it), and the scan kernel's bytes per second from its time.

    python tools/volscan_probe.py [--runs 5] [--workloads r32 r128 r8 confetti] [--e2e r32 r8] [--launches] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from nyxus_amd import _abi  # noqa: E402
from vol_probe import workload  # noqa: E402

HBM_PEAK_GBS = 8000.0                                       # bench.py's roofline peak
GRIDS = {"r32": ((128, 128, 128), 32), "r128": ((128, 256, 256), 128), "r8": ((64, 128, 128), 8)}   # (z, y, x) of the volume, cell side
NAMES = ("r32", "r128", "r8", "confetti")


def volume(name: str):
    """(I [1, z, y, x] uint16, L [1, z, y, x] uint32) of a workload."""
    if name == "confetti":
        rng = np.random.default_rng(96)
        m = 48
        labels = np.unique(rng.integers(1, 2 ** 32, size=2 * m ** 3, dtype=np.uint64))[:m ** 3].astype(np.uint32)
        rng.shuffle(labels)
        L = np.repeat(np.repeat(np.repeat(labels.reshape(m, m, m), 2, 0), 2, 1), 2, 2)
        return rng.integers(1, 4096, size=L.shape).astype(np.uint16)[None], np.ascontiguousarray(L)[None]
    shape, cell = GRIDS[name]
    b = workload(name)
    I, L = np.zeros(shape, np.uint16), np.zeros(shape, np.uint32)
    off = b.px_offset.astype(np.int64)
    nz, ny, nx = (s // cell for s in shape)
    for r in range(b.n_roi):
        cz, cy, cx = r // (ny * nx), (r // nx) % ny, r % nx
        assert cz < nz
        sl = slice(off[r], off[r + 1])
        z, y, x = cz * cell + b.z[sl].astype(np.int64), cy * cell + b.y[sl].astype(np.int64), cx * cell + b.x[sl].astype(np.int64)
        I[z, y, x] = b.inten[sl]
        L[z, y, x] = r + 1
    return I[None], L[None]


def ms(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def stat(t):
    return f"{np.median(t):9.2f} ({np.min(t):.2f} .. {np.max(t):.2f})"


def kernel_times(wname):
    """{kernel: (calls, average microseconds)} of the scan's launches on one workload, from a traced child process"""
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not prof:
        return None
    d = tempfile.mkdtemp(prefix="volscanprobe_")
    cmd = [prof, "--kernel-trace", "--stats", "-d", d, "-o", "vs", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--workloads", wname,
           "--runs", "3", "--e2e", "--device-only"]
    try:
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    except (subprocess.SubprocessError, OSError):
        return None
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            m = re.search(r"(vol_scan_kernel|vol_cloud_kernel|vs_\w+_kernel)(<.*?>)?", row.get("Name", ""))
            if m:
                tag = m.group(1) + (" (count pass)" if m.group(1) == "vol_cloud_kernel" and re.search(r"(true|\(bool\)1)>$", m.group(2) or "") else "")
                calls, avg = out.get(tag, (0, 0.0))
                c = int(row["Calls"])
                out[tag] = (calls + c, (avg * calls + float(row["AverageNs"]) / 1e3 * c) / (calls + c))
    shutil.rmtree(d, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--workloads", nargs="*", default=list(NAMES))
    ap.add_argument("--e2e", nargs="*", default=None, help="workloads of measurement (d); default: all of --workloads")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--device-only", action="store_true", help="measurement (c) alone (the traced child of --launches)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    e2e = a.workloads if a.e2e is None else a.e2e
    rows = []
    vols = {w: volume(w) for w in a.workloads}
    if a.launches:                                          # the traced children first: this process has not opened the GPU yet
        for w in a.workloads:
            kt = kernel_times(w)
            if kt is None:
                print(f"{w}: no per-launch times (rocprofv3 missing or its run failed)")
                continue
            for name, (calls, us) in sorted(kt.items()):
                rows.append({"workload": w, "kernel": name, "calls": calls, "avg_us": us})
                print(f"{w:8s} {name:34s} {calls:5d} launches  {us:10.1f} us on average", flush=True)
            if "vol_scan_kernel" in kt:
                I, L = vols[w]
                gbs = (I.nbytes + L.nbytes) / (kt["vol_scan_kernel"][1] * 1e-6) / 1e9
                print(f"{w:8s} vol_scan_kernel reads {I.nbytes + L.nbytes} bytes: {gbs:.0f} GB/s, {100 * gbs / HBM_PEAK_GBS:.1f} % of {HBM_PEAK_GBS:.0f} GB/s", flush=True)

    import torch
    from nyxus_amd import _lib
    from nyxus_amd.nyxus3d import Nyxus3DShape, clouds_from_volume
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    view = {2: np.int16, 4: np.int32, 8: np.int64}
    for w in a.workloads:
        I, L = vols[w]
        ti, tl = torch.from_numpy(I.view(np.int16)).to(dev), torch.from_numpy(L.view(np.int32)).to(dev)
        torch.cuda.synchronize()

        def host():
            b = _abi.batch3d_from_rois(clouds_from_volume(I[0], L[0]))
            keep = [torch.from_numpy(getattr(b, k).view(view[getattr(b, k).dtype.itemsize])).to(dev)
                    for k in ("px_offset", "x", "y", "z", "inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten")]
            torch.cuda.synchronize()
            return len(keep)

        calls = [("(c) dev/dev", lambda: ctx.assemble_volumes_device(ti.data_ptr(), _abi.U16, tl.data_ptr(), _abi.U32, I.shape))]
        if not a.device_only:
            calls = [("(a) host", host), ("(b) dev/host", lambda: ctx.assemble_volumes_host(I, L))] + calls
        n_roi = ctx.assemble_volumes_host(I, L).n_roi
        for _, f in calls:
            f()
        T = np.array([[ms(f) for _, f in calls] for _ in range(a.runs)])
        print(f"{w:8s} {I.shape[1]} x {I.shape[2]} x {I.shape[3]} (z, y, x), {n_roi} ROIs, {int((L != 0).sum())} labelled voxels; ms per call, median (range):")
        for k, (name, _) in enumerate(calls):
            print(f"  {name:14s} {stat(T[:, k])}", flush=True)
            rows.append({"workload": w, "rois": n_roi, "what": name, "median_ms": float(np.median(T[:, k])), "min_ms": float(T[:, k].min()), "max_ms": float(T[:, k].max())})
        gbs = (I.nbytes + L.nbytes) / (np.median(T[:, -1]) * 1e-3) / 1e9
        print(f"  (c) moves the volume's {I.nbytes + L.nbytes} bytes at {gbs:.1f} GB/s: {100 * gbs / HBM_PEAK_GBS:.2f} % of {HBM_PEAK_GBS:.0f} GB/s (the whole call)", flush=True)
        if not a.device_only:
            print(f"  (a) / (b) = {np.median(T[:, 0]) / np.median(T[:, 1]):.1f}", flush=True)
        if w in e2e and not a.device_only:
            n = Nyxus3DShape(["*3D_ALL*"], coarse_gray_depth=64)
            for k in ("3gldm/greydepth", "3ngtdm/greydepth", "3glrlm/greydepth", "3glszm/greydepth"):
                n.set_metaparam(k + "=64")
            n.set_metaparam("3ngtdm/radius=1")
            routes = [("(d) e2e host", lambda: n.featurize(I, L, assembly="host")), ("(d) e2e device", lambda: n.featurize(I, L, assembly="device"))]
            for _, f in routes:
                f()
            E = np.array([[ms(f) for _, f in routes] for _ in range(a.runs)])
            for k, (name, _) in enumerate(routes):
                print(f"  {name:14s} {stat(E[:, k])}", flush=True)
                rows.append({"workload": w, "rois": n_roi, "what": name, "median_ms": float(np.median(E[:, k])), "min_ms": float(E[:, k].min()), "max_ms": float(E[:, k].max())})
            print(f"  (d) host / device = {np.median(E[:, 0]) / np.median(E[:, 1]):.2f}", flush=True)
    ctx.close()
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
