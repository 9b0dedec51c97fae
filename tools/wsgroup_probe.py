"""Cost of nyxhip_wsgroup_slides: ms per slide and image bytes per second on stacks of 64 slides of 1024^2 and 8 of 4096^2 (uint8 and uint16),
device-resident and from host memory, each bit of the mask alone and all four; the figures as a share of the HBM rate of bench.py's
roofline, median and range of five runs after a warm-up (wall time of the synchronous call).
Beside it the comparison "one workgroup per slide": the same 1024^2 slide through the cloud route with the segmented kernels,
featurize_host(slide_batch(...), FAM_SMOMS | FAM_IMOMS | FAM_RADIAL), host memory (one slide; the route has no device-image entry).
    python tools/wsgroup_probe.py [runs] [quick]"""
import sys
import time
import numpy as np
sys.path.insert(0, ".")
import torch
from nyxus_amd import _abi, _lib
from tests.wholeslide_cases import slide_batch

HBM_PEAK_GBS = 8000.0            # bench.py's roofline figure
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
quick = len(sys.argv) > 2
dev = torch.device("cuda", 0)
ctx = _lib.Context(0)
s = _abi.default_settings(64)
MASKS = [("CONTOUR", _abi.WS_CONTOUR), ("SMOMS", _abi.WS_SMOMS), ("IMOMS", _abi.WS_IMOMS), ("RADIAL", _abi.WS_RADIAL), ("all four", _abi.WS_ALL)]


def timed(call):
    call()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def line(tag, ms, n, nbytes):
    gbs = nbytes / (ms[0] * 1e-3) / 1e9
    print(f"{tag}: median {ms[0]:.3f} ms (range {ms[1]:.3f} .. {ms[2]:.3f}) = {ms[0] / n:.4f} ms per slide, {gbs:.1f} GB/s of image bytes = "
          f"{100 * gbs / HBM_PEAK_GBS:.2f} % of the {HBM_PEAK_GBS:.0f} GB/s roofline rate", flush=True)


print(f"runs = {runs}")
for n, side in ((64, 1024), (8, 4096)):
    for dt, tdt, hi in ((np.uint8, torch.uint8, 256), (np.uint16, torch.int16, 65536)):
        g = torch.Generator(device=dev).manual_seed(n + side)
        d_in = torch.randint(0, hi, (n, side, side), generator=g, device=dev, dtype=torch.int32).to(tdt).contiguous()
        h_in = d_in.cpu().numpy().view(dt)
        nbytes = n * side * side * np.dtype(dt).itemsize
        for tag, mask in MASKS:
            ncol = _lib.load().nyxhip_wsgroup_n_columns(mask)
            d_out = torch.empty((n, ncol), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            line(f"{n} x {side}^2 {np.dtype(dt).name} device, {tag}",
                 timed(lambda: ctx.wsgroup_slides_device(d_in.data_ptr(), np.dtype(dt).itemsize, n, side, side, mask, s, d_out.data_ptr(), ncol)), n, nbytes)
            if not quick or mask == _abi.WS_ALL:
                line(f"{n} x {side}^2 {np.dtype(dt).name} host, {tag}", timed(lambda: ctx.wsgroup_slides_host(h_in, mask, s)), n, nbytes)
        if side == 1024 and dt == np.uint16:
            b = slide_batch([h_in[0]])
            fam = _abi.FAM_SMOMS | _abi.FAM_IMOMS | _abi.FAM_RADIAL
            line("1 x 1024^2 uint16 through the cloud route (one workgroup per slide), moments + radial", timed(lambda: ctx.featurize_host(b, fam, s)), 1,
                 side * side * 2)
            line("1 x 1024^2 uint16 host, SMOMS | IMOMS | RADIAL (the dense sweep on the same slide)",
                 timed(lambda: ctx.wsgroup_slides_host(h_in[:1], _abi.WS_SMOMS | _abi.WS_IMOMS | _abi.WS_RADIAL, s)), 1, side * side * 2)
        del d_in
ctx.close()
