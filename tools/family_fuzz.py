"""Fuzz every family against the oracle: random shapes, intensity distributions (narrow, wide, with zeros, huge values),
grey depths and binning modes.  Prints mismatching columns per round."""
import sys
import numpy as np
sys.path.insert(0, ".")
from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from oracle import counts
from tests import parity

ctx = _lib.Context(0)
seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rng = np.random.default_rng(seed)
total_bad = 0
for rnd in range(rounds):
    mode = rng.integers(0, 4)
    ibsi = mode == 3
    gd = int(rng.choice([2, 3, 8, 16, 64, 100, 255])) if mode != 1 else -int(rng.choice([4, 16, 32]))
    s = _abi.default_settings(gd, ibsi)
    s.glcm_n_angles = int(rng.integers(1, 5))
    s.glcm_offset = int(rng.integers(1, 4))
    rois = []
    for k in range(80):
        h, w = rng.integers(1, 48, 2)
        yy, xx = np.mgrid[0:h, 0:w]
        shape = rng.integers(0, 4)
        if shape == 0:
            m = np.ones((h, w), bool)
        elif shape == 1:
            m = (((xx - w / 2) / (w / 2 + .5)) ** 2 + ((yy - h / 2) / (h / 2 + .5)) ** 2) <= 1
        elif shape == 2:
            m = rng.random((h, w)) < 0.7
        else:
            m = (((xx - w / 2) / (w / 2 + .5)) ** 2 + ((yy - h / 2) / (h / 2 + .5)) ** 2) <= 1
            m &= rng.random((h, w)) > 0.15
        if not m.any():
            m[0, 0] = True
        ys, xs = np.nonzero(m)
        xs = xs - xs.min(); ys = ys - ys.min()
        dist = rng.integers(0, 6)
        n = len(xs)
        if ibsi:
            v = rng.integers(0 if rng.random() < .3 else 1, int(rng.choice([3, 7, 20, 60])), n)
        elif dist == 0:
            v = rng.integers(1, 4096, n)
        elif dist == 1:
            v = rng.integers(0, 10, n)
        elif dist == 2:
            v = rng.integers(60000, 65536, n)
        elif dist == 3:
            v = np.full(n, int(rng.integers(0, 1000)))
        elif dist == 4:
            v = rng.integers(0, 2 ** 32 - 1, n)
        else:
            v = (rng.normal(1000, 30, n)).clip(0).astype(np.int64)
        if ibsi and v.max() == 0:
            v[0] = 1
        rois.append(dict(x=xs, y=ys, inten=v.astype(np.uint32)))
    b = _abi.batch_from_rois(rois)
    mask = _abi.FAM_ALL & ~_abi.FAM_GABOR
    if gd < 0 and not ibsi:
        mask &= ~(_abi.FAM_GLDZM | _abi.FAM_NGLDM)
    if rnd % 5 == 0:
        mask |= _abi.FAM_GABOR
    try:
        G = ctx.featurize_host(b, mask, s)
    except _lib.NyxHipError as e:
        print("round", rnd, "gd", gd, "ibsi", ibsi, "-> error", e)
        continue
    O = po.oracle_featurize(b, mask, s)
    names = _lib.column_names(mask, s)
    bad = parity.compare_tables(G, O, names, atol=parity.moment_atol(b)) + counts.compare_counts(G, O, names) + counts.compare_tight(G, O, names)
    # ill-conditioned weighted-moment rows (w00 cancels) are reported separately
    hard = [x for x in bad if not any(t in x for t in ("WNCM", "WHU", "WT_NORM", "WEIGHTED_HU", "IMOM_WCM", "WEIGHTED_CENTRAL"))]
    total_bad += len(hard)
    print("round", rnd, "gd", gd, "ibsi", ibsi, "na", s.glcm_n_angles, "off", s.glcm_offset, "mismatches", len(bad), "hard", len(hard), hard[:3])
print("done; hard mismatches:", total_bad)
