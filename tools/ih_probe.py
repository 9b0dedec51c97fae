"""Cost of the intensity-histogram entry (nyxhip_ih_batch): ns per ROI on device-resident batches of the benchmark's ROI shapes -- disks of
49 px (radius 4) and of 2821 px (radius 30, the ROIs bench.py featurizes) -- at 12-bit and 16-bit data, on flat ROIs (one intensity but for
two extreme pixels: almost every pixel lands in two bins, the worst case of the LDS atomics) and on the heavy-tailed batch of
tests/radial_cases.heavy().  *ALL_INTENSITY* alone on the same device batch stands beside every figure for scale: it reads the same bytes
and does far more arithmetic.  Wall time of the synchronous call on a device batch (no copies), median of `reps` after a warm-up.
NYXHIP_IH_ONE_FORM=1 in the environment sends every ROI through the workgroup-per-ROI form (the A/B of the two launch forms).
    python tools/ih_probe.py [reps] [grey_depth]"""
import os
import sys
import time
import numpy as np
sys.path.insert(0, ".")
import torch
from nyxus_amd import _abi, _lib
from tests import radial_cases, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
depth = int(sys.argv[2]) if len(sys.argv) > 2 else 64
dev = torch.device("cuda", 0)
ctx = _lib.Context(0)
s = _abi.default_settings(depth, True)


def disks(radius, pitch, hi, flat=False):
    lab = synth.disk_label_tile(size=1024, pitch=pitch, radius=radius)
    it = synth.intensity_tile(3, size=1024, lo=1, hi=hi)
    rois = synth.rois_from_tile(it, lab)
    if flat:
        for r in rois:
            v = np.full(len(r["inten"]), hi // 2, np.uint32)
            v[0], v[-1] = 1, hi - 1
            r["inten"] = v
    return _abi.batch_from_rois(rois)


def on_device(b):
    keep = {k: torch.from_numpy(getattr(b, k).view({2: np.int16, 4: np.int32, 8: np.int64}[getattr(b, k).dtype.itemsize])).to(dev)
            for k in ("px_offset", "x", "y", "inten", "bbox_w", "bbox_h", "min_inten", "max_inten")}
    cb = b.c_struct()
    for k, t in keep.items():
        setattr(cb, k, t.data_ptr())
    cb.roi_label = None; cb.slide_min = None; cb.slide_max = None; cb.memory = _abi.MEM_DEVICE
    return cb, keep


def median_ms(call):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3


print(f"N = {depth} bins, reps = {reps}, NYXHIP_IH_ONE_FORM = {os.environ.get('NYXHIP_IH_ONE_FORM', '0')}")
cases = [("49-px disks, 12-bit", disks(4, 12, 4096)), ("49-px disks, 16-bit", disks(4, 12, 65536)),
         ("2821-px disks, 12-bit", disks(30, 73, 4096)), ("2821-px disks, 16-bit", disks(30, 73, 65536)),
         ("49-px disks, flat", disks(4, 12, 4096, flat=True)), ("2821-px disks, flat", disks(30, 73, 4096, flat=True)),
         ("heavy-tailed", _abi.batch_from_rois(radial_cases.heavy()))]
for tag, b in cases:
    cb, keep = on_device(b)
    out = torch.empty((b.n_roi, _abi.IH_COLS), dtype=torch.float64, device=dev)
    ih = median_ms(lambda: ctx.ih_device(cb, s, out.data_ptr(), _abi.IH_COLS))
    ncol = ctx.n_columns(_abi.FAM_INTENSITY, s)
    out2 = torch.empty((b.n_roi, ncol), dtype=torch.float64, device=dev)

    def intensity():
        ctx.featurize_device_async(cb, _abi.FAM_INTENSITY, s, out2.data_ptr(), ncol)
        ctx.sync()
    it = median_ms(intensity)
    print(f"{tag}: {b.n_roi} ROIs, {int(b.px_offset[-1])} px | IH median {ih[0]:.3f} ms (min {ih[1]:.3f}) = {ih[0] * 1e6 / b.n_roi:.0f} ns per ROI | "
          f"*ALL_INTENSITY* alone median {it[0]:.3f} ms (min {it[1]:.3f}) = {it[0] * 1e6 / b.n_roi:.0f} ns per ROI")
ctx.close()
