#!/usr/bin/env python3
"""Random volumetric ROIs through nyxhip_featurize_volumes_tex against tests/voltex_ref.py: blobs, slabs, needles and shells, box sides
1 .. 48, every binning mode (radiomics, matlab, none, IBSI), NGTDM radius 0 .. 3.  NaN and inf must sit in the same places; finite values
within --tol relative (the four variance columns against max(|value|, 1), as tests/test_voltex_gpu.py measures them).  Prints the largest
relative difference.

    python tools/voltex_fuzz.py [--batches 40] [--rois 12] [--seed 1] [--tol 1e-10]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nyxus_amd import _abi, _lib  # noqa: E402
from tests import voltex_cases, voltex_ref  # noqa: E402


def random_roi(rng, hi):
    kind = rng.choice(["blob", "slab", "needle", "shell"])
    w, h, d = (int(v) for v in rng.integers(1, 49, 3))
    if kind == "slab":
        d = int(rng.integers(1, 3))
    elif kind == "needle":
        h, d = int(rng.integers(1, 3)), int(rng.integers(1, 3))
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    keep = rng.random(x.shape) < rng.uniform(0.3, 1.0)
    if kind == "shell":
        keep &= (x == 0) | (y == 0) | (z == 0) | (x == w - 1) | (y == h - 1) | (z == d - 1)
    keep.flat[0] = keep.flat[-1] = True
    v = ((x + 2 * y + 3 * z) * hi // max(1, w + 2 * h + 3 * d) + rng.integers(0, max(2, hi // 5), x.shape)) % (hi + 1)
    if rng.random() < 0.1:
        v[:] = int(rng.integers(0, hi + 1))                 # a flat ROI
    return {"x": x[keep], "y": y[keep], "z": z[keep], "inten": v[keep].astype(np.uint32), "origin": (0, 0, 0), "box": (w, h, d)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--rois", type=int, default=12)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--tol", type=float, default=1e-10)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = _lib.Context(0)
    floor = np.array([1.0 if c in ("3GLDM_GLV", "3GLDM_DV", "3NGLDM_GLV", "3NGLDM_DCV") else 0.0 for c in voltex_cases.column_names()])
    worst, nbad = 0.0, 0
    for k in range(a.batches):
        mode = ["radiomics", "matlab", "none", "ibsi"][k % 4]
        s = _abi.default_settings(int(rng.integers(1, 129)))
        t = _abi.VolTexSettings(0, 0, int(rng.integers(0, 4)))
        hi = 4000
        if mode == "radiomics":
            t.gldm_grey_depth, t.ngtdm_grey_depth = -int(rng.integers(1, 129)), -int(rng.integers(1, 129))
        elif mode == "matlab":
            t.gldm_grey_depth, t.ngtdm_grey_depth = int(rng.integers(1, 129)), int(rng.integers(1, 129))
        else:
            hi = int(rng.integers(2, 129))                  # the levels are the intensities
            s.ibsi = 1 if mode == "ibsi" else 0
        b = _abi.batch3d_from_rois([random_roi(rng, hi) for _ in range(a.rois)])
        want = voltex_ref.table(b, s, t)
        got = ctx.volumes_tex_host(b, _abi.VTEX_ALL, s, t)
        ok = (np.isnan(got) == np.isnan(want)) & (np.isinf(got) == np.isinf(want))
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(np.isfinite(want) & (got != want), np.abs(got - want) / np.maximum(np.abs(want), floor[None, :]), 0.0)
        rel = np.where(np.isfinite(rel), rel, np.inf)
        ok &= rel <= a.tol
        worst = max(worst, float(rel[np.isfinite(rel)].max(initial=0.0)))
        if not ok.all():
            nbad += 1
            r, c = np.argwhere(~ok)[0]
            print(f"batch {k} ({mode}, grey depths {s.grey_depth} / {t.gldm_grey_depth} / {t.ngtdm_grey_depth}, radius {t.ngtdm_radius}): ROI {r} box "
                  f"{b.bbox_w[r]}x{b.bbox_h[r]}x{b.bbox_d[r]} column {voltex_cases.column_names()[c]}: got {got[r, c]!r} want {want[r, c]!r}")
    ctx.close()
    print(f"{a.batches} batches x {a.rois} ROIs: {nbad} batches with a mismatch; largest relative difference {worst:.3e}")
    sys.exit(1 if nbad else 0)


if __name__ == "__main__":
    main()
