#!/usr/bin/env python3
"""Times nyxhip_featurize_volumes_tex on device batches: wall time of the synchronous call (it ends in a stream synchronise), median of
15 after 3 warm-up calls, ms per call and ns per voxel, on the three workloads of tools/vol_probe.py -- 64 ROIs of ~32^3, 4 ROIs of
~128^3, 2000 ROIs of ~8^3 -- at grey depth 64 and NGTDM radius 1, each class alone and all three together.  --out FILE also writes the
rows as JSON.

    python tools/voltex_probe.py [--repeat 15] [--workloads r32 r128 r8] [--radius 1] [--out FILE]

The reference's side (the same ROIs through the reference's own classes on 16 CPU threads) is timed by
VOLTEXREF_TIME=1 python tests/golden/voltex/make_voltex_golden.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from nyxus_amd import _abi  # noqa: E402
from vol_probe import WORKLOADS, workload  # noqa: E402


def main():
    import torch
    from nyxus_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--workloads", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--radius", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    view = {2: np.int16, 4: np.int32, 8: np.int64}
    rows = []
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
        t = _abi.VolTexSettings(64, 64, a.radius)
        for cls, mask in (("gldm", _abi.VTEX_GLDM), ("ngldm", _abi.VTEX_NGLDM), ("ngtdm", _abi.VTEX_NGTDM), ("all", _abi.VTEX_ALL)):
            ncol = len(_lib.voltex_column_names(mask))
            out = torch.zeros((b.n_roi, ncol), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            for _ in range(3):
                ctx.volumes_tex_device(cb, mask, s, t, out.data_ptr(), ncol)
            ts = []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                ctx.volumes_tex_device(cb, mask, s, t, out.data_ptr(), ncol)   # synchronous: returns after the stream has drained
                ts.append(time.perf_counter() - t0)
            med = float(np.median(ts))
            rows.append({"workload": wname, "rois": b.n_roi, "voxels": nvox, "radius": a.radius, "class": cls, "ms_per_call": med * 1e3,
                         "ns_per_voxel": med * 1e9 / nvox, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3})
            print(f"{wname:5s} {b.n_roi:5d} ROIs {nvox:9d} voxels  radius {a.radius}  {cls:6s}  {med * 1e3:9.3f} ms per call  {med * 1e9 / nvox:8.2f} ns per voxel  "
                  f"(min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f})", flush=True)
    ctx.close()
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
