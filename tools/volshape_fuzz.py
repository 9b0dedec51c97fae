#!/usr/bin/env python3
"""Random volumetric ROIs through nyxhip_featurize_volumes_shape against tests/volshape_ref.py: blobs, shells, needles, slabs and clouds
whose corners carry intensity 0, box sides 1 .. 48.  3AREA and 6 V of the hull must agree bit for bit; 3VOXEL_VOLUME and the closed forms
within --tol relative; the eigen columns as squares ((len / 4)^2 within --tol x lambda_max, the squared ratios within --tol), as
tests/test_volshape_gpu.py measures them.  Prints the largest differences.

    python tools/volshape_fuzz.py [--batches 24] [--rois 12] [--seed 1] [--tol 1e-10]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nyxus_amd import _abi, _lib  # noqa: E402
from tests import volshape_cases, volshape_ref  # noqa: E402


def random_roi(rng):
    kind = rng.choice(["blob", "shell", "needle", "slab", "dark"])
    w, h, d = (int(v) for v in rng.integers(1, 49, 3))
    if kind == "slab":
        d = int(rng.integers(1, 3))
    elif kind == "needle":
        h, d = int(rng.integers(1, 3)), int(rng.integers(1, 3))
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    keep = rng.random(x.shape) < rng.uniform(0.2, 1.0)
    if kind == "blob":                                      # an ellipsoid inside the box, thinned
        keep &= ((2 * x + 1 - w) / w) ** 2 + ((2 * y + 1 - h) / h) ** 2 + ((2 * z + 1 - d) / d) ** 2 <= 1.0
    if kind == "shell":
        keep &= (x == 0) | (y == 0) | (z == 0) | (x == w - 1) | (y == h - 1) | (z == d - 1)
    keep.flat[0] = keep.flat[-1] = True
    v = rng.integers(1, 100, x.shape)
    if kind == "dark":                                      # the corners of the box, and a tenth of the rest, carry intensity 0
        v[(rng.random(x.shape) < 0.1) | (((x == 0) | (x == w - 1)) & ((y == 0) | (y == h - 1)) & ((z == 0) | (z == d - 1)))] = 0
    return {"x": x[keep], "y": y[keep], "z": z[keep], "inten": v[keep].astype(np.uint32), "origin": (0, 0, 0), "box": (w, h, d)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--rois", type=int, default=12)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--tol", type=float, default=1e-10)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = _lib.Context(0)
    s = _abi.default_settings(64)
    worst = {"closed": 0.0, "lens": 0.0, "ratios": 0.0}
    bad = 0
    for k in range(a.batches):
        b = _abi.batch3d_from_rois([random_roi(rng) for _ in range(a.rois)])
        got = ctx.volumes_shape_host(b, _abi.VSHAPE_MORPHOLOGY, s)
        h6 = volshape_ref.hull6_of(b)
        want = np.array([volshape_ref.row(*volshape_ref.roi_arrays(b, r), hull6=int(h6[r])) for r in range(b.n_roi)])
        fig = volshape_cases.figures(got, want)
        exact = (got[:, 0] == want[:, 0]) & (got[:, volshape_ref.HULL[0]] == h6 / 6.0) & (got[:, volshape_ref.HULL[1]] == h6 / 6.0)
        for key in worst:
            worst[key] = max(worst[key], fig[key])
        if not exact.all() or max(fig[key] for key in worst) > a.tol:
            bad += 1
            print(f"batch {k}: MISMATCH rows {np.flatnonzero(~exact).tolist()} figures {fig}; boxes {list(zip(b.bbox_w, b.bbox_h, b.bbox_d))}")
    ctx.close()
    print(f"{a.batches} batches x {a.rois} ROIs: {bad} mismatching; largest differences: closed forms {worst['closed']:.3e}, eigen squares {worst['lens']:.3e}, "
          f"squared ratios {worst['ratios']:.3e} (tolerance {a.tol:.0e}); 3AREA and 6 V bit for bit")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
