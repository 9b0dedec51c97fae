"""Cost of NYXHIP_FAM_CIRCLES and NYXHIP_FAM_GEODETIC, each alone: ns per ROI on the benchmark's ROIs (tests/synth.tile_batch, the tiles
bench.py featurizes) and on the heavy-tailed batch of tests/radial_cases.heavy(), host-to-host calls, median of `reps` after a warm-up.
Both bits pay for the contour chain (roi_contour_kernel) they read; ROI_RADIUS, which pays for it too, is printed for scale.
    python tools/circle_probe.py [reps]"""
import sys
import time
import numpy as np
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import radial_cases, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
ctx = _lib.Context(0)
s = _abi.default_settings(64)
for tag, b in (("benchmark tile", synth.tile_batch(0)), ("heavy-tailed", _abi.batch_from_rois(radial_cases.heavy()))):
    for mask, name in ((_abi.FAM_CIRCLES, "CIRCLES"), (_abi.FAM_GEODETIC, "GEODETIC"), (_abi.FAM_ROI_RADIUS, "ROI_RADIUS (for scale)")):
        ctx.featurize_host(b, mask, s)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.featurize_host(b, mask, s)
            t.append(time.perf_counter() - t0)
        t = np.array(t)
        print(f"{tag}: {b.n_roi} ROIs, {int(b.px_offset[-1])} pixels, {name}: median {np.median(t) * 1e3:.3f} ms, min {t.min() * 1e3:.3f} ms "
              f"= {np.median(t) * 1e9 / b.n_roi:.0f} ns per ROI (host call, copies included)")
