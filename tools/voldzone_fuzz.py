#!/usr/bin/env python3
"""Random volumetric ROIs through nyxhip_featurize_volumes_dzones against tests/voldzone_ref.py: blobs, slabs, needles, shells,
checkerboards and plates with holes, box sides 1 .. 48, every binning mode (radiomics, matlab, none, IBSI), few and many levels.  Under
radiomics binning the sparse clouds are what voldzone_cases.rule_excluded names: there the restatement of the ruling is
the only reference.  NaN and inf must sit in the same places; finite values within --tol relative (the variance columns against
max(|value|, 1), as tests/test_voldzone_gpu.py measures them).  Prints the largest relative difference.

    python tools/voldzone_fuzz.py [--batches 24] [--rois 12] [--seed 1] [--tol 1e-10]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nyxus_amd import _abi, _lib  # noqa: E402
from tests import voldzone_cases, voldzone_ref  # noqa: E402


def random_roi(rng, hi):
    kind = rng.choice(["blob", "slab", "needle", "shell", "checker", "plate"])
    w, h, d = (int(v) for v in rng.integers(1, 49, 3))
    if kind in ("slab", "plate"):
        d = int(rng.integers(1, 3))
    elif kind == "needle":
        h, d = int(rng.integers(1, 3)), int(rng.integers(1, 3))
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    keep = rng.random(x.shape) < rng.uniform(0.3, 1.0)
    if kind == "shell":
        keep &= (x == 0) | (y == 0) | (z == 0) | (x == w - 1) | (y == h - 1) | (z == d - 1)
    lv = int(rng.choice([2, 3, 5, hi]))                     # few levels: large zones, deep metrics
    if kind == "checker":
        v = 1 + ((x + y + z) & 1) * (hi - 1) if rng.random() < 0.5 else 1 + ((x & 1) + 2 * (y & 1) + 4 * (z & 1)) % hi
        keep[:] = True
    elif kind == "plate":                                   # one or two levels in broad bands, a few round holes: zones far from any border
        v = 1 + (x * 2 // max(1, w)) * (hi - 1)
        keep[:] = True
        for _ in range(int(rng.integers(0, 4))):
            cx, cy, rad = rng.integers(0, w), rng.integers(0, h), rng.integers(1, 4)
            keep &= (x - cx) ** 2 + (y - cy) ** 2 > rad * rad
    else:
        v = ((x + 2 * y + 3 * z) * lv // max(1, w + 2 * h + 3 * d) + rng.integers(0, max(2, lv // 2), x.shape)) % (lv + 1) * (hi // lv)
        v[rng.random(x.shape) < 0.02] = 0
    keep.flat[0] = keep.flat[-1] = True
    if rng.random() < 0.08:
        v = np.full(x.shape, int(rng.integers(0, hi + 1)))  # a flat ROI
    return {"x": x[keep], "y": y[keep], "z": z[keep], "inten": np.asarray(v)[keep].astype(np.uint32), "origin": (0, 0, 0), "box": (w, h, d)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--rois", type=int, default=12)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--tol", type=float, default=1e-10)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = _lib.Context(0)
    names = voldzone_cases.column_names()
    worst, nbad, ruled, total = 0.0, 0, 0, 0
    for k in range(a.batches):
        mode = ["radiomics", "matlab", "none", "ibsi"][k % 4]
        s = _abi.default_settings(64)
        hi = 4000
        if mode == "radiomics":
            s.grey_depth = -int(rng.integers(1, 129))
        elif mode == "matlab":
            s.grey_depth = int(rng.integers(1, 129))
        else:
            hi = int(rng.integers(2, 129))                  # the levels are the intensities
            s.grey_depth = 0 if mode == "none" else 64
            s.ibsi = 1 if mode == "ibsi" else 0
        b = _abi.batch3d_from_rois([random_roi(rng, hi) for _ in range(a.rois)])
        ruled += int(voldzone_cases.rule_excluded(b, s).sum())
        total += b.n_roi
        want = voldzone_ref.table(b, s)
        got = ctx.volumes_dzones_host(b, _abi.VDZ_GLDZM, s)
        rel = voldzone_cases.rel_diff(got, want, names)     # inf where NaN / inf sit in different places
        worst = max(worst, float(rel[np.isfinite(rel)].max(initial=0.0)))
        if not (rel <= a.tol).all():
            nbad += 1
            r, c = np.argwhere(~(rel <= a.tol))[0]
            print(f"batch {k} ({mode}, grey depth {s.grey_depth}): ROI {r} box {b.bbox_w[r]}x{b.bbox_h[r]}x{b.bbox_d[r]} "
                  f"column {names[c]}: got {got[r, c]!r} want {want[r, c]!r}")
    ctx.close()
    print(f"{a.batches} batches x {a.rois} ROIs ({ruled} of {total} ROIs rule-excluded: held to the ruling alone): {nbad} batches with a mismatch; "
          f"largest relative difference {worst:.3e}")
    sys.exit(1 if nbad else 0)


if __name__ == "__main__":
    main()
