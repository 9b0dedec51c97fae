"""Fuzz the chords kernel (NYXHIP_FAM_CHORDS) against tests/chords_ref.py on adversarial masks at random origins that include
(0, 0): noise, needles (1 x N, N x 1, slopes), combs, rings, plates with holes, masks with zero-intensity pixels (global planes,
the last pixel of the cloud decides a cell), and one thin shape per round around the size where the kernel leaves LDS.  Every
value must be bit-identical to the restatement.
    python tools/chords_fuzz.py [seed] [rounds]"""
import sys
import numpy as np
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import chords_ref
from tests.outline_cases import ring
from tests.radial_cases import comb

ctx = _lib.Context(0)
s = _abi.default_settings(8)
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
n_bad = n_rows = n_same = n_vals = 0
for rnd in range(int(sys.argv[2]) if len(sys.argv) > 2 else 10):
    rois = []
    for k in range(40):
        h, w = (int(v) for v in rng.choice([1, 2, 3, 7, 16, 31, 33, 64, 65, 90, 150, 210], 2))
        if k == 0:
            h, w = int(rng.choice([1, 3])), int(rng.choice([505, 508, 509, 510, 511, 600]))   # one thin shape at the LDS limit per round
        kind = rng.integers(0, 6)
        yy, xx = np.mgrid[0:h, 0:w]
        if kind == 0:                                                 # plate with random rectangular holes
            m = np.ones((h, w), bool)
            for _ in range(int(rng.integers(0, 5))):
                y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w)); m[y0:y0 + int(rng.integers(1, 6)), x0:x0 + int(rng.integers(1, 6))] = False
        elif kind == 1:                                               # ring
            m = np.zeros((h, w), bool); r = ring(); m[:r.shape[0], :r.shape[1]] = r[:h, :w]
        elif kind == 2:                                               # needle along a random slope
            m = yy == (xx * max(h - 1, 0)) // max(w - 1, 1)
        elif kind == 3:
            m = rng.random((h, w)) < rng.choice([0.02, 0.3, 0.7, 0.95])
        elif kind == 4:
            m = comb(max(w // 4, 1), max(h - 6, 1))[:h, :w] if h > 6 and w >= 4 else np.ones((h, w), bool)
        else:                                                         # diagonal band + specks
            m = (np.abs(xx - yy) <= 1) | (rng.random((h, w)) < 0.05)
        if not m.any():
            m[0, 0] = True
        ys, xs = np.nonzero(m)
        o = rng.permutation(len(xs)) if rng.random() < 0.3 else np.lexsort((ys, xs))
        ox, oy = (int(v) for v in rng.choice([0, 0, 1, 977, 4093, 65536, 1_000_003, 2 ** 31], 2))
        v = rng.integers(1, 500, len(xs)).astype(np.uint32)
        if rng.random() < 0.3:                                        # zero-intensity pixels: holes, and a question of order
            v[rng.random(len(xs)) < rng.choice([0.02, 0.3, 1.0])] = 0
        rois.append(dict(x=xs[o] + ox, y=ys[o] + oy, inten=v))
    b = _abi.batch_from_rois(rois)
    G = ctx.featurize_host(b, _abi.FAM_CHORDS, s)
    O = chords_ref.table(b)
    n_rows += b.n_roi; n_same += int((G == O).sum()); n_vals += G.size
    bad = [f"row {r} {chords_ref.NAMES[c]}: got {G[r, c]!r}, want {O[r, c]!r}" for r, c in np.argwhere(G != O)[:10]]
    if bad:
        n_bad += len(bad)
        print("round", rnd, bad[:5])
print(f"{n_rows} ROIs, {n_same} of {n_vals} values bit-identical, {n_bad} mismatches")
sys.exit(1 if n_bad else 0)
