#!/usr/bin/env python3
"""Random stacks through nyxhip_assemble_volumes against the host assembly (clouds_from_volume + batch3d_from_rois): blobs, shells,
needles, interleaved checkerboards and confetti in volumes of sides 1 .. 48 (the seams of the scan block and of the slab form of the
cloud launch over-sampled through a wide, flat or deep variant), every pair of element types, random 32-bit label values, host and
device memory, random budgets that cut host stacks into chunks.  Every array of the batch, the volume indices and the stated extrema are
compared bit for bit.  Exit code 1 on the first difference.

    python tools/volscan_fuzz.py [--rounds 200] [--seed 1] [--dump DIR]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nyxus_amd import _abi, _lib  # noqa: E402
from tests import volscan_cases as vc  # noqa: E402
from tests.test_volscan_gpu import check_assembled, to_device  # noqa: E402

DT = (np.uint8, np.uint16, np.uint32)


def sides(rng):
    """(z, y, x): mostly 1 .. 48 each; one in four rounds sits on a seam: the column seam, the row seam, or a box above the slab threshold"""
    d, h, w = (int(rng.integers(1, 49)) for _ in range(3))
    k = rng.integers(0, 12)
    if k == 0:
        w, h, d = vc.SCAN_COLS + int(rng.integers(-2, 3)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
    elif k == 1:
        h, w = vc.SCAN_ROWS + int(rng.integers(-1, 2)), int(rng.integers(1, 9))
    elif k == 2:
        w, h, d = 32 + int(rng.integers(0, 3)), 32 + int(rng.integers(0, 3)), vc.SLAB_CELLS // 1024 + int(rng.integers(-1, 3))
    return d, h, w


def labels_of(rng, n, dt):
    hi = np.iinfo(dt).max
    pool = np.unique(np.concatenate([rng.integers(1, hi + 1, size=4 * n + 8, dtype=np.uint64), [1, hi, hi // 2 + 1]]))
    return rng.permutation(pool)[:n].astype(np.uint32)


def paint(rng, L, dt):
    """one random figure into the label volume L [z, y, x]"""
    d, h, w = L.shape
    kind = rng.integers(0, 6)
    z0, y0, x0 = (int(rng.integers(0, s)) for s in L.shape)
    z1, y1, x1 = (int(rng.integers(a + 1, s + 1)) for a, s in ((z0, d), (y0, h), (x0, w)))
    box = L[z0:z1, y0:y1, x0:x1]
    lab = labels_of(rng, 2, dt)
    if kind == 0:                                            # blob: a random half of a box
        box[rng.random(box.shape) < 0.5] = lab[0]
    elif kind == 1:                                          # shell around a blob of another label
        box[...] = lab[0]
        if min(box.shape) > 2:
            box[1:-1, 1:-1, 1:-1] = lab[1]
    elif kind == 2:                                          # needle along one axis
        ax = int(rng.integers(0, 3))
        idx = [z0, y0, x0]
        idx[ax] = slice(None)
        L[tuple(idx)] = lab[0]
    elif kind == 3:                                          # two labels interleaved as a checkerboard
        z, y, x = np.indices(box.shape)
        box[...] = np.where((z + y + x) % 2 == 0, lab[0], lab[1])
    elif kind == 4:                                          # confetti: every voxel of a box its own label (as far as the type has values)
        vals = labels_of(rng, min(box.size, int(np.iinfo(dt).max)), dt)
        zz, yy, xx = np.unravel_index(rng.permutation(box.size)[:len(vals)], box.shape)
        box[zz, yy, xx] = vals
    else:                                                    # one label in two far corners
        L[0, 0, 0] = lab[0]
        L[-1, -1, -1] = lab[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dump", default=None, help="directory that receives the volumes of a failing round")
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(a.seed)
    ctx = _lib.Context(0)
    n_roi = n_chunked = 0
    for r in range(a.rounds):
        di, dl = DT[rng.integers(0, 3)], DT[rng.integers(0, 3)]
        d, h, w = sides(rng)
        nv = int(rng.integers(1, 4))
        L = np.zeros((nv, d, h, w), np.uint32)
        for v in range(nv):
            for _ in range(int(rng.integers(0, 5))):
                paint(rng, L[v], dl)
        I = rng.integers(0, int(np.iinfo(di).max) + 1, size=L.shape, dtype=np.uint64).astype(di)
        I[rng.random(L.shape) < 0.1] = 0
        L = L.astype(dl)
        b, vol = vc.host_assembly(I, L)
        what = f"round {r}: {nv} x {d} x {h} x {w}, {np.dtype(di).name} / {np.dtype(dl).name}, {b.n_roi} ROIs"
        try:
            mode = rng.integers(0, 3)
            if mode == 0:
                check_assembled(ctx.assemble_volumes_host(I, L), b, vol, what=what)
            elif mode == 1:
                ti, tl = to_device(I), to_device(L)
                torch.cuda.synchronize()
                check_assembled(ctx.assemble_volumes_device(ti.data_ptr(), _abi.volume_dtype(di), tl.data_ptr(), _abi.volume_dtype(dl), I.shape), b, vol, what=what)
            else:                                            # a budget of one to three volumes with the largest tables they can grow to
                cap = 1
                while cap < 2 * d * h * w:
                    cap <<= 1
                budget = int(rng.integers(1, 4)) * (vc.chunk_bytes(I.shape[1:], di, dl) + 4 * vc.TABLE_WORDS * max(cap, vc.CAP_MIN))
                check_assembled(ctx.assemble_volumes_host(I, L, max_device_bytes=budget), b, vol, budget, what=what)
                n_chunked += 1
        except AssertionError as e:
            print("DIFFERENCE", what, str(e)[:2000])
            if a.dump:
                np.savez(os.path.join(a.dump, f"volscan_fuzz_fail_{a.seed}_{r}.npz"), I=I, L=L)
            sys.exit(1)
        n_roi += b.n_roi
    ctx.close()
    print(f"volscan_fuzz: {a.rounds} rounds, {n_roi} ROIs, {n_chunked} rounds under a budget: every array equal bit for bit")


if __name__ == "__main__":
    main()
