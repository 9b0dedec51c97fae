"""Cost of the four bits of the morphology entries, each alone and all four: ns per ROI on the benchmark's ROIs (tests/synth.tile_batch,
the tiles bench.py featurizes: one tile, and 64 times its ROIs in one batch) and on the heavy-tailed batch of tests/radial_cases.heavy().  Device-resident batches with stated extrema,
so a call is the launches and their read-backs alone; median of `reps` after a warm-up.  NYXHIP_MORPH_CONTOUR and NYXHIP_MORPH_HULL pay
for the contour chain (roi_contour_kernel) they read: NYXHIP_FAM_ROI_RADIUS of nyxhip_featurize_batch, which pays for it too, is printed
for scale.  For BASIC | EXTREMA (the cloud sweeps alone) the cloud's bytes per second are printed as well: 8 B per pixel in sweep 1, 4 B in
each of the two distance sweeps.
    python tools/morph_probe.py [reps]"""
import sys
import time
import numpy as np
import torch
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import radial_cases, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
ctx = _lib.Context(0)
s = _abi.default_settings(64)
dev = torch.device("cuda", 0)
view = {2: np.int16, 4: np.int32, 8: np.int64}
_it, _lab = synth.intensity_tile(0, size=1024), synth.disk_label_tile(size=1024, irregular=False, seed=0)
_tile_rois = synth.rois_from_tile(_it, _lab)
# one benchmark tile (a call of 196 ROIs is bound by launch latency and its read-backs) | 64 times its ROIs (the rate of the kernels) | heavy-tailed
for tag, b in (("benchmark tile", synth.tile_batch(0)), ("64 benchmark tiles", _abi.batch_from_rois(_tile_rois * 64)),
               ("heavy-tailed", _abi.batch_from_rois(radial_cases.heavy()))):
    keep = {k: torch.from_numpy(getattr(b, k).view(view[getattr(b, k).dtype.itemsize])).to(dev)
            for k in ("roi_label", "px_offset", "x", "y", "inten", "bbox_w", "bbox_h", "min_inten", "max_inten")}
    h = b.c_struct()
    cb = _abi.Batch()
    cb.n_roi = b.n_roi
    for k, t in keep.items():
        setattr(cb, k, t.data_ptr())
    cb.memory = _abi.MEM_DEVICE
    cb.max_px, cb.max_bbox_area, cb.max_bbox_side = h.max_px, h.max_bbox_area, h.max_bbox_side
    out = torch.zeros((b.n_roi, 64), dtype=torch.float64, device=dev)
    npx = int(b.px_offset[-1])
    calls = [(f"MORPH {name}", (lambda m=m: ctx.morph_device(cb, None, None, m, s, out.data_ptr(), 64)), m)
             for m, name in ((1, "BASIC"), (2, "CONTOUR"), (4, "HULL"), (8, "EXTREMA"), (9, "BASIC | EXTREMA"), (15, "ALL"))]
    for name, call, m in calls:
        call()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            t.append(time.perf_counter() - t0)
        t = np.array(t)
        line = (f"{tag}: {b.n_roi} ROIs, {npx} pixels, {name}: median {np.median(t) * 1e3:.3f} ms, min {t.min() * 1e3:.3f} ms "
                f"= {np.median(t) * 1e9 / b.n_roi:.0f} ns per ROI (device batch, synchronous call)")
        if m == 9:
            line += f"; cloud bytes {16 * npx} -> {16 * npx / np.median(t) / 1e9:.1f} GB/s"
        print(line)
    hb = b
    ctx.featurize_host(hb, _abi.FAM_ROI_RADIUS, s)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.featurize_host(hb, _abi.FAM_ROI_RADIUS, s)
        t.append(time.perf_counter() - t0)
    print(f"{tag}: ROI_RADIUS (contour chain + one reader, HOST batch with its copies, for scale): median {np.median(t) * 1e3:.3f} ms")
