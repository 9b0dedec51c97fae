"""Fuzz the morphology kernel (nyxhip_morph_batch and nyxhip_morph_tiles, every mask) against tests/morph_ref.py: random masks of
several densities, needles, combs, rings and plates with holes at random origins (with (0, 0)); box sides 1 .. 300 with the bounds of
the kernel's paths over-sampled (the ballot words, the 8192-cell LDS plane, and -- one box per round -- the 1024-column LDS table).
38 columns must be bit-identical to the restatement; COMPACTNESS, EDGE_MEAN_INTENSITY and EDGE_STDDEV_INTENSITY are held to
parity.REL_TOL.  Prints the largest relative difference per column.
    python tools/morph_fuzz.py [seed] [rounds]"""
import sys
import numpy as np
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import morph_ref, parity
from tests.outline_cases import ring
from tests.radial_cases import comb

ctx = _lib.Context(0)
s = _abi.default_settings(8)
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
N = morph_ref.NAMES
ROUNDED = [N.index(c) for c in morph_ref.ROUNDED]
worst = np.zeros(41)
n_bad = n_rows = 0
SIDES = [1, 2, 3, 4, 5, 7, 16, 31, 33, 63, 64, 65, 90, 91, 128, 129, 140, 300]


def mask_of(kind, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 0:
        m = np.ones((h, w), bool)
        if h > 6 and w > 6:
            m[h // 3:h // 3 + max(h // 4, 1), w // 3:w // 3 + max(w // 4, 1)] = False           # a plate with a hole
    elif kind == 1:
        m = np.zeros((h, w), bool); r = ring(); m[:r.shape[0], :r.shape[1]] = r[:h, :w]
    elif kind == 2:
        m = yy == (xx * max(h - 1, 0)) // max(w - 1, 1)                                         # needle along a slope
    elif kind == 3:
        m = rng.random((h, w)) < rng.choice([0.3, 0.7, 0.95])
    elif kind == 4:
        m = comb(max(w // 4, 1), max(h - 2, 1), spine=2)[:h, :w] if h > 2 and w >= 4 else np.ones((h, w), bool)
    else:
        m = (xx - w / 2) ** 2 * h * h + (yy - h / 2) ** 2 * w * w <= (w * h / 2) ** 2           # ellipse
    if not m.any():
        m[0, 0] = True
    return m


def check(tag, G, O, mask):
    global n_bad
    cols = morph_ref.columns_of(mask)
    O = O[:, cols]
    with np.errstate(invalid="ignore"):
        rel = np.where(G == O, 0.0, np.abs(G - O) / np.maximum(np.abs(O), 1e-300))
    for k, c in enumerate(cols):
        worst[c] = max(worst[c], rel[:, k].max())
        lim = parity.REL_TOL if c in ROUNDED else 0.0
        rows_bad = np.nonzero(~(rel[:, k] <= lim))[0]
        if len(rows_bad):
            n_bad += len(rows_bad)
            print(tag, f"mask {mask:#x} {N[c]}: row {rows_bad[0]} got {G[rows_bad[0], k]!r}, want {O[rows_bad[0], k]!r}")


for rnd in range(int(sys.argv[2]) if len(sys.argv) > 2 else 10):
    rois = []
    for k in range(24):
        h, w = (int(v) for v in rng.choice(SIDES, 2))
        if k == 0:
            h, w = int(rng.integers(1, 4)), int(rng.choice([1023, 1024, 1025, 1500]))           # the LDS column-table bound
        m = mask_of(int(rng.integers(0, 6)), h, w)
        ys, xs = np.nonzero(m)
        o = np.lexsort((ys, xs))
        v = rng.integers(0, int(rng.choice([2, 500, 2 ** 32])), len(xs)).astype(np.uint32)
        ox, oy = ((0, 0), (int(rng.integers(0, 70000)), int(rng.integers(0, 70000))), (int(rng.integers(0, 2 ** 20)), int(rng.integers(0, 2 ** 20))))[int(rng.integers(0, 3))]
        rois.append(dict(x=xs[o] + ox, y=ys[o] + oy, inten=v))
    b = _abi.batch_from_rois(rois)
    O = morph_ref.table(b)
    n_rows += b.n_roi
    for mask in (15, int(rng.integers(1, 16))):
        check(f"round {rnd} batch", ctx.morph_host(b, mask, s), O, mask)
    # the tile entry: some of the shapes pasted into one label image, rows in label order
    H = W = 512
    it, lab = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
    placed, x0, y0, row_h = [], 1, 1, 0
    for r in rois[1:]:
        rx, ry = r["x"] - r["x"].min(), r["y"] - r["y"].min()
        bw, bh = int(rx.max()) + 1, int(ry.max()) + 1
        if x0 + bw + 1 > W:
            x0, y0, row_h = 1, y0 + row_h + 1, 0
        if y0 + bh + 1 > H:
            break
        lab[ry + y0, rx + x0] = len(placed) + 1
        it[ry + y0, rx + x0] = r["inten"]
        placed.append(dict(x=rx + x0, y=ry + y0, inten=r["inten"]))
        x0, row_h = x0 + bw + 1, max(row_h, bh)
    tb = _abi.batch_from_rois(placed)
    mask = int(rng.integers(1, 16))
    tiles, labels, T = ctx.morph_tiles_host(it[None], lab[None], mask, s)
    assert list(labels) == list(range(1, len(placed) + 1)), "tile rows"
    check(f"round {rnd} tile", T, morph_ref.table(tb), mask)
    n_rows += tb.n_roi
print("largest relative difference per column:", {N[c]: float(worst[c]) for c in range(41) if worst[c] > 0})
print(f"{n_rows} ROIs, {n_bad} mismatches")
sys.exit(1 if n_bad else 0)
