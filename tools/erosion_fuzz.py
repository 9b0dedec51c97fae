"""Fuzz the erosion and ellipse kernels (NYXHIP_FAM_EROSION | NYXHIP_FAM_ELLIPSE) against tests/erosion_ref.py: random masks of
several densities, needles, combs, rings, filled boxes (fixed points: 1000 without 1000 passes), bridged checkerboards, boxes around
the word boundaries (31 .. 33, 63 .. 65 columns) and the empty-loop sizes (< 4), constant ROIs (skipped), and one box per round
beyond the LDS planes.  The erosion columns and every ellipse column but ORIENTATION (atan) must be bit-identical to the
restatement; ORIENTATION within 1e-12 of it.
    python tools/erosion_fuzz.py [seed] [rounds]"""
import sys
import numpy as np
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import erosion_ref
from tests.outline_cases import ring
from tests.radial_cases import comb

ctx = _lib.Context(0)
s = _abi.default_settings(8)
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
n_bad = n_rows = 0
for rnd in range(int(sys.argv[2]) if len(sys.argv) > 2 else 10):
    rois = []
    for k in range(40):
        h, w = (int(v) for v in rng.choice([1, 2, 3, 4, 5, 7, 16, 31, 32, 33, 63, 64, 65, 90, 150], 2))
        if k == 0:
            h, w = int(rng.choice([130, 300, 420])), int(rng.choice([1000, 1023, 1024, 1025]))   # beyond the LDS planes
        kind = rng.integers(0, 7)
        yy, xx = np.mgrid[0:h, 0:w]
        if kind == 0:
            m = np.ones((h, w), bool)                                 # filled box
        elif kind == 1:
            m = np.zeros((h, w), bool); r = ring(); m[:r.shape[0], :r.shape[1]] = r[:h, :w]
        elif kind == 2:
            m = yy == (xx * max(h - 1, 0)) // max(w - 1, 1)           # needle along a slope
        elif kind == 3:
            m = rng.random((h, w)) < rng.choice([0.3, 0.7, 0.95, 0.995])
        elif kind == 4:
            m = comb(max(w // 4, 1), max(h - 6, 1))[:h, :w] if h > 6 and w >= 4 else np.ones((h, w), bool)
        elif kind == 5:
            m = ((xx + yy) % 2 == 0) | (yy % 5 == 0)                  # bridged checkerboard
        else:
            m = (xx - w / 2) ** 2 * h * h + (yy - h / 2) ** 2 * w * w <= (w * h / 2) ** 2   # ellipse
        if not m.any():
            m[0, 0] = True
        ys, xs = np.nonzero(m)
        o = rng.permutation(len(xs)) if rng.random() < 0.3 else np.lexsort((ys, xs))
        v = rng.integers(0, 500, len(xs)).astype(np.uint32)
        if rng.random() < 0.1:
            v[:] = 9                                                  # constant: the erosion class is skipped
        rois.append(dict(x=xs[o], y=ys[o], inten=v))
    b = _abi.batch_from_rois(rois)
    G = ctx.featurize_host(b, _abi.FAM_ELLIPSE | _abi.FAM_EROSION, s)
    O = erosion_ref.table(b)
    n_rows += b.n_roi
    ok = G == O
    ok[:, 4] = np.abs(G[:, 4] - O[:, 4]) <= 1e-12 * np.maximum(np.abs(O[:, 4]), 1.0)
    bad = [f"row {r} {erosion_ref.NAMES[c]}: got {G[r, c]!r}, want {O[r, c]!r}" for r, c in np.argwhere(~ok)[:10]]
    if bad:
        n_bad += len(bad)
        print("round", rnd, bad[:5])
print(f"{n_rows} ROIs, {n_bad} mismatches")
sys.exit(1 if n_bad else 0)
