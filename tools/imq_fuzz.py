"""Fuzzer of the image-quality entries against tests/imq_ref.py: random masks, needles, combs, rings, flat and bimodal patches, box sides
1 .. 300 with the switch-overs (kImqWaveCells, kImqLdsCells, a wave's 64 columns) over-sampled, intensity ranges from a handful of levels
up to 32 bits; every round goes through nyxhip_imq_batch (a host batch) and nyxhip_imq_tiles (the same ROIs painted onto one tile, rows bit
for bit those of the batch), and random slides go through nyxhip_imq_slides (bit for bit nyxhip_imq_batch on the equivalent one-ROI batch).
Saturation bit for bit, the two focus columns within parity.REL_TOL (an exact 0 where the restatement has 0); prints the largest relative
difference seen on the focus columns.
    python tools/imq_fuzz.py [rounds] [seed]"""
import sys
import numpy as np
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import imq_cases, imq_ref, parity

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 30
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rng = np.random.default_rng(seed)
ctx = _lib.Context(0)
s = imq_cases.settings()
bad = 0
worst = 0.0
n_rows = 0
SIDES = [1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 119, 120, 121, 127, 128, 129, 255, 256, 257, 300]


def side():
    return int(rng.choice(SIDES)) if rng.random() < 0.5 else int(rng.integers(1, 301))


def box():
    """(w, h): half of the boxes sit on a switch-over -- w * h within a row of kImqWaveCells or kImqLdsCells."""
    w, h = side(), side()
    if rng.random() < 0.3:
        target = int(rng.choice([imq_cases.WAVE_CELLS, imq_cases.LDS_CELLS]))
        h = max(1, min(300, (target + int(rng.integers(-1, 2)) * w) // w))
    return w, h


def mask_of(w, h):
    kind = int(rng.integers(0, 7))
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 0:                                         # filled
        m = np.ones((h, w), bool)
    elif kind == 1:                                       # random
        m = rng.random((h, w)) < rng.uniform(0.05, 0.95)
    elif kind == 2:                                       # needle: a diagonal
        m = (xx * max(h - 1, 1) == yy * max(w - 1, 1)) | (xx * h // max(w, 1) == yy)
    elif kind == 3:                                       # comb
        m = (xx % 2 == 0) | (yy == 0)
    elif kind == 4:                                       # ring
        cy, cx, ry, rx = (h - 1) / 2, (w - 1) / 2, max(h / 2, 0.5), max(w / 2, 0.5)
        d = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
        m = (d <= 1.0) & (d >= 0.5)
    elif kind == 5:                                       # disc
        cy, cx, ry, rx = (h - 1) / 2, (w - 1) / 2, max(h / 2, 0.5), max(w / 2, 0.5)
        m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    else:                                                 # a frame
        m = (xx == 0) | (yy == 0) | (xx == w - 1) | (yy == h - 1)
    # the box must be the box: its four sides are touched
    m[0, int(rng.integers(0, w))] = True; m[h - 1, int(rng.integers(0, w))] = True
    m[int(rng.integers(0, h)), 0] = True; m[int(rng.integers(0, h)), w - 1] = True
    return m


def values(n):
    kind = int(rng.integers(0, 6))
    top = int(rng.choice([2, 4, 9, 256, 4096, 65536, 2 ** 32 - 1]))
    lo = int(rng.integers(0, max(1, top // 2)))
    if kind == 0:                                         # flat but for a few pixels
        v = np.full(n, lo + (top - lo) // 2, np.uint64)
        k = int(rng.integers(0, min(n, 4) + 1))
        v[rng.integers(0, n, k)] = rng.integers(lo, top, k, dtype=np.uint64)
    elif kind == 1:                                       # bimodal: the extremes
        v = np.where(rng.random(n) < 0.5, lo, top).astype(np.uint64)
    elif kind == 2:                                       # a single intensity (0 now and then)
        v = np.full(n, 0 if rng.random() < 0.3 else lo, np.uint64)
    else:
        v = rng.integers(lo, top + 1, n, dtype=np.uint64)
    return v.astype(np.uint32)


def compare(tag, got, want):
    global bad, worst
    ok = imq_ref.same_bits(got[:, imq_ref.SATURATION], want[:, imq_ref.SATURATION])
    rel = imq_ref.rel_diff(got[:, imq_ref.FOCUS], want[:, imq_ref.FOCUS])
    fin = rel[np.isfinite(rel)]
    worst = max(worst, float(fin.max()) if fin.size else 0.0)
    if not ok.all() or (rel > parity.REL_TOL).any():
        bad += 1
        print(f"MISMATCH {tag}: saturation rows {np.argwhere(~ok)[:6].tolist()}, focus rows {np.argwhere(rel > parity.REL_TOL)[:6].tolist()}, "
              f"largest relative difference {rel.max():.3e}")


for k in range(rounds):
    # ---- ROIs side by side on one tile, and the same ROIs as a host batch -----------------------------------------------------------------
    rois, x0, H = [], 1, 0
    for _ in range(int(rng.integers(3, 12))):
        w, h = box()
        m = mask_of(w, h)
        ys, xs = np.nonzero(m)
        rois.append({"x": xs + x0, "y": ys + 1, "inten": values(len(xs)), "label": len(rois) + 1})
        x0 += w + 1
        H = max(H, h + 2)
    b = _abi.batch_from_rois(rois)
    want = imq_ref.table(b, s)
    got = ctx.imq_host(b, s)
    compare(f"round {k} batch", got, want)
    lab = np.zeros((1, H, x0 + 1), np.uint32)
    it = np.zeros((1, H, x0 + 1), np.uint32)
    for r in rois:
        lab[0, r["y"], r["x"]] = r["label"]
        it[0, r["y"], r["x"]] = r["inten"]
    tiles, labels, T = ctx.imq_tiles_host(it, lab, s)
    if list(labels) != [r["label"] for r in rois] or not imq_ref.same_bits(T, got).all():
        bad += 1
        print(f"MISMATCH round {k}: the tile entry and the batch entry differ")
    n_rows += b.n_roi
    # ---- slides ------------------------------------------------------------------------------------------------------------------------------
    dtype = [np.uint8, np.uint16, np.uint32][k % 3]
    w, h = side(), side()
    n = int(rng.integers(1, 4))
    top = int(rng.choice([2, 200, np.iinfo(dtype).max]))
    st = rng.integers(0, min(top, np.iinfo(dtype).max) + 1, (n, h, w), dtype=np.uint64).astype(dtype)
    if rng.random() < 0.2:
        st[0][:] = st[0, 0, 0]
    sb = imq_cases.slide_batch(st)
    want = ctx.imq_host(sb, s)
    compare(f"round {k} slides {w} x {h} {np.dtype(dtype).name}, batch entry", want, imq_ref.table(sb, s))
    got = ctx.imq_slides_host(st, s, max_device_bytes=0 if k % 2 else 4 * st[0].nbytes + (1 << 16))
    if not imq_ref.same_bits(got, want).all():
        bad += 1
        print(f"MISMATCH round {k}: slides {w} x {h} {np.dtype(dtype).name} differ from the batch entry", got, want)
    n_rows += n
print(f"{rounds} rounds, {n_rows} rows, {bad} mismatches; largest relative difference on the focus columns {worst:.3e}")
ctx.close()
sys.exit(1 if bad else 0)
