"""Fuzz the circle kernel (NYXHIP_FAM_CIRCLES | NYXHIP_FAM_GEODETIC) against tests/circle_ref.py: random masks of several densities,
needles, combs, rings, spirals and plates with holes at random origins (with (0, 0), and some beyond 2^24 where (float) x rounds).
All five columns must be bit-identical to the restatement.
    python tools/circle_fuzz.py [seed] [rounds]"""
import sys
import numpy as np
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import circle_cases, circle_ref
from tests.outline_cases import ring
from tests.radial_cases import comb

ctx = _lib.Context(0)
s = _abi.default_settings(8)
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
n_bad = n_rows = 0
for rnd in range(int(sys.argv[2]) if len(sys.argv) > 2 else 10):
    rois = []
    for k in range(32):
        h, w = (int(v) for v in rng.choice([1, 2, 3, 4, 5, 7, 16, 31, 33, 64, 90, 140], 2))
        kind = rng.integers(0, 7)
        yy, xx = np.mgrid[0:h, 0:w]
        if kind == 0:
            m = np.ones((h, w), bool)
            if h > 6 and w > 6:
                m[h // 3:h // 3 + max(h // 4, 1), w // 3:w // 3 + max(w // 4, 1)] = False       # a plate with a hole
        elif kind == 1:
            m = np.zeros((h, w), bool); r = ring(); m[:r.shape[0], :r.shape[1]] = r[:h, :w]
        elif kind == 2:
            m = yy == (xx * max(h - 1, 0)) // max(w - 1, 1)           # needle along a slope
        elif kind == 3:
            m = rng.random((h, w)) < rng.choice([0.3, 0.7, 0.95])
        elif kind == 4:
            m = comb(max(w // 4, 1), max(h - 2, 1), spine=2)[:h, :w] if h > 2 and w >= 4 else np.ones((h, w), bool)
        elif kind == 5:
            m = circle_cases.spiral(turns=float(rng.uniform(1.0, 4.0)), step=float(rng.uniform(2.2, 4.0)))
        else:
            m = (xx - w / 2) ** 2 * h * h + (yy - h / 2) ** 2 * w * w <= (w * h / 2) ** 2   # ellipse
        if not m.any():
            m[0, 0] = True
        ys, xs = np.nonzero(m)
        o = np.lexsort((ys, xs))
        v = rng.integers(1, 500, len(xs)).astype(np.uint32)
        ox, oy = ((0, 0), (int(rng.integers(0, 70000)), int(rng.integers(0, 70000))), (int(rng.integers(2 ** 24, 2 ** 24 + 4000)), int(rng.integers(0, 2 ** 25))))[int(rng.integers(0, 3))]
        rois.append(dict(x=xs[o] + ox, y=ys[o] + oy, inten=v))
    b = _abi.batch_from_rois(rois)
    G = ctx.featurize_host(b, _abi.FAM_CIRCLES | _abi.FAM_GEODETIC, s)
    O = circle_ref.table(b)[:, :5]
    n_rows += b.n_roi
    bad = [f"row {r} {circle_ref.NAMES[c]}: got {G[r, c]!r}, want {O[r, c]!r}" for r, c in np.argwhere(G != O)[:10]]
    if bad:
        n_bad += len(bad)
        print("round", rnd, bad[:5])
print(f"{n_rows} ROIs, {n_bad} mismatches")
sys.exit(1 if n_bad else 0)
