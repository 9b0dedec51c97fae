#!/usr/bin/env python3
"""Fuzzes nyxhip_featurize_volumes against tests/vol_ref.py: random blobs, needles, slabs, shells and flat patches with box sides 1 .. 48,
every binning mode of the GLCM block (radiomics, matlab, matlab symmetric, IBSI), offsets 1 .. 3, 8- to 32-bit intensities.  Compared under
the project's policy (vol_cases.compare: integer-valued and order-statistic columns bit for bit, the rest within parity.REL_TOL).

    python tools/vol_fuzz.py [--rounds 40] [--seed 1]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nyxus_amd import _abi, _lib  # noqa: E402
from tests import vol_cases, vol_ref  # noqa: E402


def shape(rng, kind, ibsi):
    side = lambda: int(rng.integers(1, 49))
    w, h, d = side(), side(), side()
    if kind == "needle":
        w, h, d = [(side(), 1, 1), (1, side(), 1), (1, 1, side())][int(rng.integers(3))]
    elif kind == "slab":
        w, h, d = [(side(), side(), 1), (side(), 1, side()), (1, side(), side())][int(rng.integers(3))]
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    if kind == "blob":
        keep = rng.random(x.shape) < rng.uniform(0.2, 1.0)
    elif kind == "shell":
        keep = (x == 0) | (y == 0) | (z == 0) | (x == w - 1) | (y == h - 1) | (z == d - 1)
    else:
        keep = np.ones(x.shape, bool)
    keep[0, 0, 0] = keep[-1, -1, -1] = True
    top = int(rng.choice([100, 127])) if ibsi else int(rng.choice([255, 4095, 65535, 2 ** 32 - 1]))
    lo = int(rng.integers(0, max(1, top // 2)))
    v = rng.integers(lo, top + 1, x.shape, dtype=np.uint64).astype(np.uint32)
    if kind == "flat":
        v[:] = v.flat[0]
    return {"x": x[keep], "y": y[keep], "z": z[keep], "inten": v[keep], "origin": (0, 0, 0), "box": (w, h, d)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = _lib.Context(0)
    worst_i = worst_g = 0.0
    for rnd in range(a.rounds):
        mode = ["radiomics", "matlab", "matlab_sym", "ibsi"][rnd % 4]
        s = _abi.default_settings(int(rng.choice([8, 64, 100])))
        s.glcm_grey_depth = {"radiomics": -1, "matlab": 1, "matlab_sym": 1, "ibsi": 1}[mode] * int(rng.choice([2, 16, 64, 128]))
        s.glcm_symmetric = int(mode == "matlab_sym")
        s.ibsi = int(mode == "ibsi")
        s.glcm_offset = int(rng.integers(1, 4))
        s.soft_nan = float(rng.choice([0.0, -9.0]))
        b = _abi.batch3d_from_rois([shape(rng, k, s.ibsi) for k in rng.choice(["blob", "needle", "slab", "shell", "flat"], int(rng.integers(1, 9)))])
        got = ctx.volumes_host(b, _abi.VFAM_ALL, s, stated=bool(rnd & 1))
        want = vol_ref.table(b, s)
        bad, ri, rg = vol_cases.compare(got, want)
        worst_i, worst_g = max(worst_i, ri), max(worst_g, rg)
        if bad:
            print(f"round {rnd} ({mode}, depth {s.glcm_grey_depth}, offset {s.glcm_offset}): MISMATCH", bad[:8], list(zip(b.bbox_w, b.bbox_h, b.bbox_d)))
            sys.exit(1)
        print(f"round {rnd}: {mode:10s} depth {s.glcm_grey_depth:4d} offset {s.glcm_offset} {b.n_roi} ROIs ok", flush=True)
    print(f"{a.rounds} rounds ok; largest relative difference: intensity block {worst_i:.3e}, GLCM block {worst_g:.3e}")
    ctx.close()


if __name__ == "__main__":
    main()
