#!/usr/bin/env python3
"""Whole-slide mode against the only route that served such rows before it: an all-ones label image through nyxhip_featurize_tiles_v2.

Seeded 12-bit data (the top eight bits for uint8) in 64 slides of 1024 x 1024 and 8 slides of 4096 x 4096, as uint8, uint16 and uint32;
*ALL_INTENSITY* + *ALL_GLCM* at grey depth 8 and 64.  Per configuration, for host arrays and for device-resident arrays: both routes in
one process, warmed up, alternating, each timed by a host clock around the synchronous call.  Prints ms per slide and pixels per
second of both routes (median of the repeats, with the spread), their ratio, and whether the two tables are bit-equal.

    python tools/wholeslide_probe.py [--reps 5] [--out probe.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nyxus_amd import _abi, _lib  # noqa: E402

MASK = _abi.FAM_INTENSITY | _abi.FAM_GLCM
TORCH_DT = {1: "uint8", 2: "int16", 4: "int32"}


def slides(n, side, dtype, seed):
    a = np.random.default_rng(seed).integers(0, 4096, (n, side, side), dtype=np.uint16)
    return np.ascontiguousarray((a >> 4).astype(np.uint8) if dtype == np.uint8 else a.astype(dtype))


def same_bits(a, b):
    return bool(a.shape == b.shape and ((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="1024:64,4096:8")
    args = ap.parse_args()
    import torch
    ctx = _lib.Context(0)
    lib = _lib.load()
    results = []
    for size_n in args.sizes.split(","):
        side, n = (int(v) for v in size_n.split(":"))
        label = np.ones((n, side, side), np.uint8)                           # the smallest label type
        d_label = torch.from_numpy(label).to("cuda:0")
        for dtype in (np.uint8, np.uint16, np.uint32):
            I = slides(n, side, dtype, seed=side + np.dtype(dtype).itemsize)
            isz = np.dtype(dtype).itemsize
            d_I = torch.from_numpy(I.view(getattr(np, TORCH_DT[isz]))).to("cuda:0")
            for gd in (8, 64):
                s = _abi.default_settings(gd)
                ncol = ctx.n_columns(MASK, s)
                d_out_t = torch.zeros((n, ncol), dtype=torch.float64, device="cuda:0")
                d_out_s = torch.zeros((n, ncol), dtype=torch.float64, device="cuda:0")
                d_lab = torch.zeros(n, dtype=torch.int32, device="cuda:0")
                d_til = torch.zeros(n, dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()

                def tiles_host():
                    return ctx.featurize_tiles_host(I, label, MASK, s, slide_mode=_abi.SLIDE_PER_TILE)[2]

                def slides_host():
                    return ctx.featurize_slides_host(I, MASK, s)

                def tiles_device():
                    t = _abi.Tiles()
                    t.inten = d_I.data_ptr(); t.label = d_label.data_ptr(); t.inten_dtype = isz; t.label_dtype = _abi.U8
                    t.width = side; t.height = side; t.n_tiles = n; t.memory = _abi.MEM_DEVICE; t.slide_mode = _abi.SLIDE_PER_TILE
                    cnt = C.c_uint64(0)
                    ctx._check(lib.nyxhip_featurize_tiles_v2(ctx._h, C.byref(t), MASK, C.byref(s), C.c_void_p(d_lab.data_ptr()), C.c_void_p(d_til.data_ptr()), n,
                                                             C.c_void_p(d_out_t.data_ptr()), ncol, C.byref(cnt)))
                    assert cnt.value == n
                    return d_out_t

                def slides_device():
                    ctx.featurize_slides_device(d_I.data_ptr(), isz, n, side, side, MASK, s, d_out_s.data_ptr(), ncol)
                    return d_out_s

                for form, f_tiles, f_slides in (("host", tiles_host, slides_host), ("device", tiles_device, slides_device)):
                    tab_t, tab_s = f_tiles(), f_slides()                     # warm-up: workspaces grow, kernels load
                    tt, ts = [], []
                    for _ in range(args.reps):
                        ms, tab_t = timed(f_tiles); tt.append(ms)
                        ms, tab_s = timed(f_slides); ts.append(ms)
                    if form == "device":
                        tab_t, tab_s = tab_t.cpu().numpy(), tab_s.cpu().numpy()
                    mt, msl = float(np.median(tt)), float(np.median(ts))
                    r = {"side": side, "slides": n, "dtype": np.dtype(dtype).name, "grey_depth": gd, "form": form,
                         "tiles_ms_per_slide": mt / n, "tiles_ms_min_max": [min(tt) / n, max(tt) / n], "tiles_px_per_s": n * side * side / (mt * 1e-3),
                         "slides_ms_per_slide": msl / n, "slides_ms_min_max": [min(ts) / n, max(ts) / n], "slides_px_per_s": n * side * side / (msl * 1e-3),
                         "ratio_tiles_over_slides": mt / msl, "bit_equal": same_bits(np.ascontiguousarray(tab_t), np.ascontiguousarray(tab_s))}
                    results.append(r)
                    print("%4d^2 x %2d %-6s gd %2d %-6s | all-ones label %8.4f ms/slide (%.4f..%.4f) %7.2f Gpx/s | whole-slide %8.4f ms/slide (%.4f..%.4f) %7.2f Gpx/s"
                          " | ratio %5.2f | bit-equal %s" % (side, n, r["dtype"], gd, form, r["tiles_ms_per_slide"], *r["tiles_ms_min_max"], r["tiles_px_per_s"] / 1e9,
                                                             r["slides_ms_per_slide"], *r["slides_ms_min_max"], r["slides_px_per_s"] / 1e9,
                                                             r["ratio_tiles_over_slides"], r["bit_equal"]), flush=True)
            del d_I
        del d_label
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
