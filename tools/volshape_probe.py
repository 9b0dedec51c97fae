#!/usr/bin/env python3
"""Times nyxhip_featurize_volumes_shape on device batches: wall time of the synchronous call (it ends in a stream synchronise), median of
15 after 3 warm-up calls, ms per call and ns per voxel, on the three workloads of tools/vol_probe.py -- 64 ROIs of ~32^3, 4 ROIs of
~128^3, 2000 ROIs of ~8^3.  Every workload is timed twice: as it is ("shape"), and with every intensity set to 0 ("nohull"), which leaves
the hull kernel no candidate to wrap -- the difference is what the convex hull costs.  --out FILE also writes the rows as JSON.

    python tools/volshape_probe.py [--repeat 15] [--workloads r32 r128 r8] [--launches] [--out FILE]

--launches also gives the time of each launch of the chain (scatter, faces, hull, close): it runs this script once more per workload as a
child process under `rocprofv3 --kernel-trace --stats` and prints the per-kernel averages of the vsh_* kernels from its statistics file
(skipped with a note where rocprofv3 is missing).

The reference's side (the same ROIs through the reference's own class on 16 CPU threads) is timed by
VOLSHAPEREF_TIME=1 python tests/golden/volshape/make_volshape_golden.py.
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
from vol_probe import WORKLOADS, workload  # noqa: E402


def kernel_times(wname, repeat):
    """{kernel name: (calls, average microseconds)} of the vsh_* kernels of one workload, from a traced child process"""
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not prof:
        return None
    d = tempfile.mkdtemp(prefix="vshprobe_")
    cmd = [prof, "--kernel-trace", "--stats", "-d", d, "-o", "vsh", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--workloads", wname,
           "--repeat", str(repeat)]
    try:
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    except (subprocess.SubprocessError, OSError):
        return None
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            m = re.search(r"(vsh_\w+)", row.get("Name", ""))
            if m:
                out[m.group(1)] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3)
    shutil.rmtree(d, ignore_errors=True)
    return out


def main():
    import torch
    from nyxus_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--workloads", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    if a.launches:                                          # the traced children first: this process has not opened the GPU yet
        for wname in a.workloads:
            kt = kernel_times(wname, 3)
            if kt is None:
                print(f"{wname}: no per-launch times (rocprofv3 missing or its run failed)")
                continue
            for name, (calls, us) in sorted(kt.items()):
                rows.append({"workload": wname, "kernel": name, "calls": calls, "avg_us": us})
                print(f"{wname:5s} {name:28s} {calls:5d} launches  {us:10.1f} us on average", flush=True)
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    view = {2: np.int16, 4: np.int32, 8: np.int64}
    for wname in a.workloads:
        b = workload(wname)
        keep = {k: torch.from_numpy(getattr(b, k).view(view[getattr(b, k).dtype.itemsize])).to(dev)
                for k in ("px_offset", "x", "y", "z", "inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten")}
        h = b.c_struct(stated=True)
        cb = _abi.Batch3D()
        cb.n_roi = b.n_roi
        for k, v in keep.items():
            setattr(cb, k, v.data_ptr())
        cb.memory = _abi.MEM_DEVICE
        cb.max_px, cb.max_bbox_cells, cb.max_inten_range = h.max_px, h.max_bbox_cells, h.max_inten_range
        nvox = int(b.px_offset[-1])
        s = _abi.default_settings(64)
        ncol = _abi.VOLSHAPE_COLS
        out = torch.zeros((b.n_roi, ncol), dtype=torch.float64, device=dev)
        for label in ("shape", "nohull"):
            if label == "nohull":                           # no voxel of non-zero intensity: the hull has no candidates
                keep["inten"].zero_()
            torch.cuda.synchronize()
            for _ in range(3):
                ctx.volumes_shape_device(cb, _abi.VSHAPE_MORPHOLOGY, s, out.data_ptr(), ncol)
            ts = []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                ctx.volumes_shape_device(cb, _abi.VSHAPE_MORPHOLOGY, s, out.data_ptr(), ncol)   # synchronous: returns after the stream has drained
                ts.append(time.perf_counter() - t0)
            med = float(np.median(ts))
            rows.append({"workload": wname, "rois": b.n_roi, "voxels": nvox, "class": label, "ms_per_call": med * 1e3, "ns_per_voxel": med * 1e9 / nvox,
                         "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3})
            print(f"{wname:5s} {b.n_roi:5d} ROIs {nvox:9d} voxels  {label:7s} {med * 1e3:9.3f} ms per call  {med * 1e9 / nvox:8.2f} ns per voxel  "
                  f"(min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f})", flush=True)
    ctx.close()
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
