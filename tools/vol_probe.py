#!/usr/bin/env python3
"""Times nyxhip_featurize_volumes on device batches: wall time of the synchronous call (it ends in a stream synchronise), median of 15
after 3 warm-up calls, ms per call and ns per voxel, for three workloads -- 64 ROIs of ~32^3, 4 ROIs of ~128^3, 2000 ROIs of ~8^3 -- at
GLCM grey depth 64 and at the level cap, each family alone and both together.  --out FILE also writes the rows as JSON.

    python tools/vol_probe.py [--repeat 15] [--workloads r32 r128 r8] [--out FILE]

The reference's side (the same ROIs through the reference's own classes on 16 CPU threads) is timed by
VOLREF_TIME=1 python tests/golden/vol/make_vol_golden.py, which imports `workload` from here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nyxus_amd import _abi  # noqa: E402

WORKLOADS = {"r32": (64, 32), "r128": (4, 128), "r8": (2000, 8)}


def workload(name: str) -> _abi.HostBatch3D:
    """n ROIs: ellipsoidal blobs (about half of their box) of 12-bit values, a ramp plus noise; sides within 10 % of the nominal one."""
    n, side = WORKLOADS[name]
    rng = np.random.default_rng(1000 + side)
    rois = []
    for _ in range(n):
        w, h, d = (int(side * f) for f in rng.uniform(0.9, 1.0, 3))
        z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
        inside = ((2 * x + 1 - w) / w) ** 2 + ((2 * y + 1 - h) / h) ** 2 + ((2 * z + 1 - d) / d) ** 2 <= 1.0
        inside[0, 0, 0] = inside[-1, -1, -1] = True
        v = (200 + (x + y + z) * 3000 // (w + h + d) + rng.integers(0, 600, x.shape)).astype(np.uint32)
        rois.append({"x": x[inside], "y": y[inside], "z": z[inside], "inten": v[inside], "origin": (0, 0, 0), "box": (w, h, d)})
    return _abi.batch3d_from_rois(rois)


def main():
    import torch
    from nyxus_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--workloads", nargs="*", default=list(WORKLOADS))
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
        for k, t in keep.items():
            setattr(cb, k, t.data_ptr())
        cb.memory = _abi.MEM_DEVICE
        cb.max_px, cb.max_bbox_cells, cb.max_inten_range = h.max_px, h.max_bbox_cells, h.max_inten_range
        nvox = int(b.px_offset[-1])
        for gd in (64, _abi.VOL_GLCM_MAX_LEVELS):
            s = _abi.default_settings(64)
            s.glcm_grey_depth = gd
            for fam, mask in (("intensity", _abi.VFAM_INTENSITY), ("glcm", _abi.VFAM_GLCM), ("both", _abi.VFAM_ALL)):
                if fam == "intensity" and gd != 64:
                    continue                                # the intensity block does not read the GLCM grey depth
                ncol = len(_lib.vol_column_names(mask, s))
                out = torch.zeros((b.n_roi, ncol), dtype=torch.float64, device=dev)
                torch.cuda.synchronize()
                for _ in range(3):
                    ctx.volumes_device(cb, mask, s, out.data_ptr(), ncol)
                ts = []
                for _ in range(a.repeat):
                    t0 = time.perf_counter()
                    ctx.volumes_device(cb, mask, s, out.data_ptr(), ncol)   # synchronous: returns after the stream has drained
                    ts.append(time.perf_counter() - t0)
                med = float(np.median(ts))
                rows.append({"workload": wname, "rois": b.n_roi, "voxels": nvox, "glcm_grey_depth": gd, "family": fam, "ms_per_call": med * 1e3,
                             "ns_per_voxel": med * 1e9 / nvox, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3})
                print(f"{wname:5s} {b.n_roi:5d} ROIs {nvox:9d} voxels  grey depth {gd:3d}  {fam:9s}  {med * 1e3:9.3f} ms per call  {med * 1e9 / nvox:8.2f} ns per voxel  "
                      f"(min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f})", flush=True)
    ctx.close()
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
