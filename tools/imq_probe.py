"""Cost of the image-quality entries.
nyxhip_imq_batch: ns per ROI on device-resident batches of the benchmark's ROI shapes -- disks of 49 px (radius 4) and of 2821 px (radius
30, the ROIs bench.py featurizes) -- and on the heavy-tailed batch of tests/radial_cases.heavy(); *ALL_INTENSITY* alone on the same device
batch stands beside every figure for scale.  Wall time of the synchronous call on a device batch (no copies), median of `reps` after a
warm-up.
nyxhip_imq_slides: ms per slide and bytes per second on device-resident stacks of 64 slides of 1024^2 and 8 of 4096^2 (uint8 and uint16),
as a share of the HBM rate of bench.py's roofline.
    python tools/imq_probe.py [reps]"""
import sys
import time
import numpy as np
sys.path.insert(0, ".")
import torch
from nyxus_amd import _abi, _lib
from tests import radial_cases, synth

HBM_PEAK_GBS = 8000.0            # bench.py's roofline figure
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
dev = torch.device("cuda", 0)
ctx = _lib.Context(0)
s = _abi.default_settings(256)


def disks(radius, pitch, hi):
    lab = synth.disk_label_tile(size=1024, pitch=pitch, radius=radius)
    it = synth.intensity_tile(3, size=1024, lo=1, hi=hi)
    return _abi.batch_from_rois(synth.rois_from_tile(it, lab))


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


print(f"reps = {reps}")
cases = [("49-px disks, 12-bit", disks(4, 12, 4096)), ("2821-px disks, 16-bit", disks(30, 73, 65536)),
         ("heavy-tailed", _abi.batch_from_rois(radial_cases.heavy()))]
for tag, b in cases:
    cb, keep = on_device(b)
    out = torch.empty((b.n_roi, _abi.IMQ_COLS), dtype=torch.float64, device=dev)
    iq = median_ms(lambda: ctx.imq_device(cb, s, out.data_ptr(), _abi.IMQ_COLS))
    ncol = ctx.n_columns(_abi.FAM_INTENSITY, s)
    out2 = torch.empty((b.n_roi, ncol), dtype=torch.float64, device=dev)

    def intensity():
        ctx.featurize_device_async(cb, _abi.FAM_INTENSITY, s, out2.data_ptr(), ncol)
        ctx.sync()
    it = median_ms(intensity)
    print(f"{tag}: {b.n_roi} ROIs, {int(b.px_offset[-1])} px | image quality median {iq[0]:.3f} ms (min {iq[1]:.3f}) = {iq[0] * 1e6 / b.n_roi:.0f} ns per ROI | "
          f"*ALL_INTENSITY* alone median {it[0]:.3f} ms (min {it[1]:.3f}) = {it[0] * 1e6 / b.n_roi:.0f} ns per ROI")

for n, side in ((64, 1024), (8, 4096)):
    for dt, tdt, hi in ((np.uint8, torch.uint8, 256), (np.uint16, torch.int16, 65536)):
        g = torch.Generator(device=dev).manual_seed(n + side)
        d_in = torch.randint(0, hi, (n, side, side), generator=g, device=dev, dtype=torch.int32).to(tdt).contiguous()
        d_out = torch.empty((n, _abi.IMQ_COLS), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ms = median_ms(lambda: ctx.imq_slides_device(d_in.data_ptr(), np.dtype(dt).itemsize, n, side, side, s, d_out.data_ptr(), _abi.IMQ_COLS))
        nbytes = n * side * side * np.dtype(dt).itemsize
        gbs = nbytes / (ms[0] * 1e-3) / 1e9
        print(f"{n} slides of {side}^2 {np.dtype(dt).name}: median {ms[0]:.3f} ms (min {ms[1]:.3f}) = {ms[0] / n:.4f} ms per slide, {gbs:.1f} GB/s of image bytes = "
              f"{100 * gbs / HBM_PEAK_GBS:.2f} % of the {HBM_PEAK_GBS:.0f} GB/s roofline rate")
ctx.close()
