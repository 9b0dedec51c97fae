"""Fuzz the radial distribution kernel (NYXHIP_FAM_RADIAL) against tests/radial_ref.py on adversarial masks: spirals, combs,
checkerboards with 8-connected bridges, noise, and exact discs (where k^2 / 49 ring ratios and diagonal wedge boundaries are
dense).  FRAC_AT_D / MEAN_FRAC must match bit for bit, RADIAL_CV within parity.REL_TOL.  ROIs on which the reference is
undefined (a centre with max_sqdist 0) are counted and must come back as 24 zeros.
    python tools/radial_fuzz.py [seed] [rounds]"""
import sys
import numpy as np
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import parity, radial_ref

ctx = _lib.Context(0)
s = _abi.default_settings(8)
mask = _abi.FAM_RADIAL
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
n_bad = n_undef = n_rows = 0


def spiral(h, w):
    m = np.zeros((h, w), bool)
    y0, y1, x0, x1 = 0, h - 1, 0, w - 1
    while y0 <= y1 and x0 <= x1:
        m[y0, x0:x1 + 1] = True; m[y0:y1 + 1, x1] = True
        if y1 - y0 >= 2: m[y1, x0 + 2:x1 + 1] = True
        if x1 - x0 >= 2 and y1 - y0 >= 2: m[y0 + 2:y1 + 1, x0 + 2] = True
        y0 += 2; x0 += 2; y1 -= 2; x1 -= 2
    return m


for rnd in range(int(sys.argv[2]) if len(sys.argv) > 2 else 10):
    rois = []
    for k in range(120):
        h, w = rng.integers(1, 48, 2)
        kind = rng.integers(0, 7)
        yy, xx = np.mgrid[0:h, 0:w]
        if kind == 0:
            m = spiral(h, w)
        elif kind == 1:                                               # comb
            m = np.zeros((h, w), bool); m[0:max(1, h // 6)] = True; m[:, ::int(rng.integers(2, 5))] = True
        elif kind == 2:                                               # checkerboard, bridged diagonally, with a few straight bridges
            m = ((xx + yy) % 2 == 0) | (rng.random((h, w)) < 0.08)
        elif kind == 3:                                               # exact disc
            r = int(rng.integers(1, 24)); yy, xx = np.mgrid[-r:r + 1, -r:r + 1]; m = xx * xx + yy * yy <= r * r
        elif kind == 4:
            m = rng.random((h, w)) < rng.choice([0.3, 0.5, 0.7, 0.9])
        elif kind == 5:                                               # ring
            r = np.hypot(xx - w / 2, yy - h / 2); m = (r < min(h, w) / 2) & (r > min(h, w) / 4)
        else:                                                         # diagonal band + specks
            m = (np.abs(xx - yy) <= 1) | (rng.random((h, w)) < 0.05)
        if not m.any():
            m[0, 0] = True
        ys, xs = np.nonzero(m)
        o = rng.permutation(len(xs)) if rng.random() < 0.3 else np.lexsort((ys, xs))     # some in a scrambled pixel order
        rois.append(dict(x=xs[o], y=ys[o], inten=rng.integers(0, rng.choice([8, 500, 2 ** 32 - 1]), len(xs)).astype(np.uint32)))
    b = _abi.batch_from_rois(rois)
    G = ctx.featurize_host(b, mask, s)
    O, D = radial_ref.radial_table(b, with_dst2=True)
    undef = np.array([d == 0 for d in D])
    n_undef += int(undef.sum()); n_rows += b.n_roi
    if undef.any() and (G[undef] != 0).any():
        print("round", rnd, "an undefined ROI did not come back as zeros"); n_bad += 1
    bad = parity.compare_tables(G, O, radial_ref.NAMES, exact=radial_ref.EXACT)
    if bad:
        n_bad += len(bad)
        print("round", rnd, bad[:5])
print(f"{n_rows} ROIs, {n_undef} undefined in the reference, {n_bad} mismatches")
sys.exit(1 if n_bad else 0)
