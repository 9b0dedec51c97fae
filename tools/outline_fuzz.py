"""Fuzz the outline kernel (NYXHIP_FAM_FRACTAL | _EULER | _ROI_RADIUS) against tests/outline_ref.py on adversarial masks: rings,
plates with holes, checkerboards with 8-connected bridges, noise, one-pixel lines, and boxes around the sides where the kernel
switches paths (32 | 33: shifting grids | one grid and a word boundary of the bit plane; 64 | 65).  EULER_NUMBER, ROI_RADIUS_MAX
and ROI_RADIUS_MEDIAN must match bit for bit, the rest within the bounds of tests/outline_cases.py.  ROIs on which the reference is
undefined (a one-point contour) are counted and not compared.
    python tools/outline_fuzz.py [seed] [rounds]"""
import sys
import numpy as np
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from tests import outline_cases, outline_ref, parity

ctx = _lib.Context(0)
s = _abi.default_settings(8)
mask = _abi.FAM_FRACTAL | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
n_bad = n_undef = n_rows = 0
for rnd in range(int(sys.argv[2]) if len(sys.argv) > 2 else 10):
    rois = []
    for k in range(100):
        h, w = (int(v) for v in rng.choice([1, 2, 3, 7, 16, 31, 32, 33, 40, 63, 64, 65, 70], 2))
        kind = rng.integers(0, 6)
        yy, xx = np.mgrid[0:h, 0:w]
        if kind == 0:                                                 # plate with random rectangular holes
            m = np.ones((h, w), bool)
            for _ in range(int(rng.integers(0, 5))):
                y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w)); m[y0:y0 + int(rng.integers(1, 6)), x0:x0 + int(rng.integers(1, 6))] = False
        elif kind == 1:                                               # checkerboard, bridged
            m = ((xx + yy) % 2 == 0) | (rng.random((h, w)) < 0.08)
        elif kind == 2:                                               # ring
            r = np.hypot(xx - w / 2, yy - h / 2); m = (r < min(h, w) / 2) & (r > min(h, w) / 4)
        elif kind == 3:
            m = rng.random((h, w)) < rng.choice([0.3, 0.5, 0.7, 0.95])
        elif kind == 4:                                               # a full box
            m = np.ones((h, w), bool)
        else:                                                         # diagonal band + specks
            m = (np.abs(xx - yy) <= 1) | (rng.random((h, w)) < 0.05)
        if not m.any():
            m[0, 0] = True
        ys, xs = np.nonzero(m)
        o = rng.permutation(len(xs)) if rng.random() < 0.3 else np.lexsort((ys, xs))
        rois.append(dict(x=xs[o], y=ys[o], inten=rng.integers(1, 500, len(xs)).astype(np.uint32)))
    b = _abi.batch_from_rois(rois)
    G = ctx.featurize_host(b, mask, s)
    O = outline_ref.outline_table(b)
    n_undef += int(np.isnan(O[:, 3]).sum()); n_rows += b.n_roi
    bad = outline_cases.mismatches(G, O, parity.REL_TOL)
    if bad:
        n_bad += len(bad)
        print("round", rnd, bad[:5])
print(f"{n_rows} ROIs, {n_undef} undefined in the reference, {n_bad} mismatches")
sys.exit(1 if n_bad else 0)
