"""Fuzzer of the intensity-histogram entries against tests/ih_ref.py: random ROIs (1 .. 3000 px), random intensity ranges (a handful of
levels up to 32 bits), flat and bimodal patches, N in {2, 3, 6, 24, 64, 256, 4096}; every round goes through nyxhip_ih_batch (a host batch)
and through nyxhip_ih_tiles (the same ROIs painted onto tiles).  Bit for bit on ih_ref.EXACT, parity.REL_TOL on the two entropy columns.
    python tools/ih_fuzz.py [rounds] [seed]"""
import sys
import numpy as np
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import ih_ref, parity, synth

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 40
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rng = np.random.default_rng(seed)
ctx = _lib.Context(0)
EX = [ih_ref.NAMES.index(c) for c in ih_ref.EXACT]
EN = [ih_ref.NAMES.index(c) for c in ih_ref.ENTROPY]
DEPTHS = (2, 3, 6, 24, 64, 256, 4096)
bad = 0
worst = 0.0
n_rows = 0


def values(n):
    kind = rng.integers(0, 6)
    top = int(rng.choice([4, 9, 256, 4096, 65536, 2 ** 32 - 1]))
    lo = int(rng.integers(0, max(1, top // 2)))
    if kind == 0:                                         # flat but for a few pixels
        v = np.full(n, lo + (top - lo) // 2, np.uint64)
        k = rng.integers(0, min(n, 4) + 1)
        v[rng.integers(0, n, k)] = rng.integers(lo, top, k, dtype=np.uint64)
    elif kind == 1:                                       # bimodal
        v = np.where(rng.random(n) < 0.5, lo, top - 1).astype(np.uint64)
        v = v + rng.integers(0, 2, n).astype(np.uint64) * (v < top - 1)
    elif kind == 2:                                       # a single intensity: gated
        v = np.full(n, lo, np.uint64)
    else:
        v = rng.integers(lo, top, n, dtype=np.uint64)
    return v.astype(np.uint32)


def compare(tag, got, want):
    global bad, worst
    ok = ih_ref.same(got[:, EX], want[:, EX])
    a, w = got[:, EN], want[:, EN]
    rel = np.where(ih_ref.same(a, w), 0.0, np.abs(a - w) / np.maximum(np.abs(w), 1e-300))
    worst = max(worst, float(rel.max()) if rel.size else 0.0)
    if not ok.all() or (rel > parity.REL_TOL).any():
        bad += 1
        print(f"MISMATCH {tag}:", [(r, ih_ref.EXACT[c], got[r, EX[c]], want[r, EX[c]]) for r, c in np.argwhere(~ok)[:6]], float(rel.max()))


for k in range(rounds):
    s = _abi.default_settings(64, True)
    s.grey_depth = int(DEPTHS[k % len(DEPTHS)])
    s.soft_nan = -7777.0
    # ---- a tile of rectangles, and the same ROIs as a host batch ------------------------------------------------------------
    size = 192
    lab = np.zeros((size, size), np.uint32)
    it = np.zeros((size, size), np.uint32)
    y = 0
    label = 0
    while y < size - 2:
        h = int(rng.integers(1, 56))
        x = 0
        while x < size - 2:
            w = int(rng.integers(1, 56))
            hh, ww = min(h, size - y), min(w, size - x)
            label += int(rng.integers(1, 50))
            lab[y:y + hh, x:x + ww] = label
            it[y:y + hh, x:x + ww] = values(hh * ww).reshape(hh, ww)
            x += ww + int(rng.integers(0, 3))
        y += h + int(rng.integers(0, 3))
    b = _abi.batch_from_rois(synth.rois_from_tile(it, lab))
    want = ih_ref.table(b, s)
    compare(f"round {k} batch N={s.grey_depth}", ctx.ih_host(b, s), want)
    tiles, labels, T = ctx.ih_tiles_host(it[None], lab[None], s)
    if list(labels) != list(b.roi_label):
        bad += 1
        print(f"MISMATCH round {k}: labels of the tile entry")
    else:
        compare(f"round {k} tiles N={s.grey_depth}", T, want)
    n_rows += 2 * b.n_roi
print(f"{rounds} rounds, {n_rows} rows, {bad} mismatches; largest relative difference on the entropy columns {worst:.3e}")
ctx.close()
sys.exit(1 if bad else 0)
