"""GPU test of the marginals of the 8-level GLCM feature launch (roi_features.hip: glcm_features_wave8 -- eight lanes per angle, two
ROIs per wave; a lane owns a row, a column and a diagonal pair of the count matrix and sums them word by word).

Every feature of the launch is a function of those sums: the row and column sums (sum_p, the means, HX), the |x - y| diagonals
(CONTRAST, DIS, the difference columns) and the x + y anti-diagonals (the sum columns).  What can go wrong lives where the order is
not 8: rows that are not 16 bytes long, lanes beyond the order, anti-diagonals that wrap; in a matrix with one occupied cell in a
corner (one lane carries everything, the longest and the shortest diagonal); in an angle without a pair (sum_p = 0); and in a wave
whose two ROIs have different orders -- the grey depth is one per call, so orders differ as 0 (a degenerate ROI: the launch skips
it) and the call's depth.  Grey depths 2, 3, 5, 7 and 8, the angle subsets {0}, {45, 135} and all four, boxes of 17 x 20.  All
columns are held to the oracle (tests/parity.py), the 24 rational GLCM columns also to the exact reference of
tests/glcm_exact_ref.py under its derived bound."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import device_call as dc
from tests import glcm_exact_ref as gx
from tests import parity

pytestmark = pytest.mark.gpu

W, H = 17, 20
DEPTHS = (2, 3, 5, 7, 8)
ANGLES = ((0,), (45, 135), (0, 45, 90, 135))
# L: a live ROI (order = the grey depth), F: a flat one (one value: the guard fires, order 0).  Slots 2k and 2k + 1 share a wave of
# the feature launch: every pairing of the two kinds occurs, in both orders
PATTERN = "LFFLLLFFLF"


def _full(values):
    k = np.arange(W * H)
    return dict(x=k // H, y=k % H, inten=np.asarray(values, np.uint32))


def _corner(low, high):
    """One pixel of `high` whose eight neighbours are not part of the ROI, everything else `low`: the only pairs are low-low, so the
    matrix has one occupied cell -- (1, 1) for a low background, (Ng, Ng) for a high one -- while the extrema span every level."""
    k = np.arange(W * H)
    x, y = k // H, k % H
    keep = ~((np.abs(x - 8) <= 1) & (np.abs(y - 10) <= 1)) | ((x == 8) & (y == 10))
    v = np.where((x == 8) & (y == 10), high, low)
    return dict(x=x[keep], y=y[keep], inten=v[keep].astype(np.uint32))


def _rois(seed):
    rng = np.random.default_rng(seed)
    rois = []
    for c in PATTERN:
        rois.append(_full(rng.integers(1, 4096, W * H)) if c == "L" else _full(np.full(W * H, int(rng.integers(1, 4096)))))
    rois += [_corner(1, 4095), _corner(4095, 1)]
    k = np.arange(40)
    rois.append(dict(x=np.zeros(40, np.int64), y=k, inten=rng.integers(1, 4096, 40).astype(np.uint32)))   # one column: pairs at 90 only
    rois.append(dict(x=k, y=np.zeros(40, np.int64), inten=rng.integers(1, 4096, 40).astype(np.uint32)))   # one row: pairs at 0 only
    rois.append(_full(rng.integers(1, 3, W * H)))                                                          # two values, 1 and 2: two levels (one at depth 2: flat)
    return rois


_cache = {}


def _batch():
    if "b" not in _cache:
        _cache["b"] = _abi.batch_from_rois(_rois(77))
    return _cache["b"]


def _settings(gd, angles):
    s = _abi.default_settings(gd)
    s.glcm_n_angles = len(angles)
    for i, a in enumerate(angles):
        s.glcm_angles[i] = a
    return s


def test_batch_shape():
    b = _batch()
    n = np.diff(b.px_offset)
    side = np.maximum(b.bbox_w, b.bbox_h)
    assert ((n > 256) | (side > 32)).all()                             # nobody in the smallest size class: the four-wave builds and their feature launch
    flat = np.asarray(b.min_inten) == np.asarray(b.max_inten)
    assert "".join("F" if f else "L" for f in flat[:len(PATTERN)]) == PATTERN and not flat[len(PATTERN):].any()
    assert n[len(PATTERN)] == W * H - 8 and b.bbox_w[-3] == 1 and b.bbox_h[-2] == 1
    s = _settings(8, ANGLES[2])
    for r, cell in ((len(PATTERN), 0), (len(PATTERN) + 1, 7)):         # the corner ROIs: one occupied cell, at (1, 1) and at (8, 8)
        plane = gx.dense_plane(b, r)
        idx, I, _ = gx.levels_of(plane, int(b.min_inten[r]), int(b.max_inten[r]), s)
        M = gx.cooc_matrix(idx, len(I), 1, 0, False)
        assert len(I) == 8 and np.count_nonzero(M) == 1 and M[cell, cell] > 0


INT_GLCM = _abi.FAM_INTENSITY | _abi.FAM_GLCM
# every depth x every subset with the intensity block beside it; GLCM alone runs the same feature launch: three of the fifteen
CASES = [(INT_GLCM, gd, a) for gd in DEPTHS for a in ANGLES] + [(_abi.FAM_GLCM, 8, ANGLES[2]), (_abi.FAM_GLCM, 5, ANGLES[1]), (_abi.FAM_GLCM, 3, ANGLES[0])]


@pytest.mark.parametrize("mask,gd,angles", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_marginals_at_every_order(hip_ctx, mask, gd, angles):
    b, s = _batch(), _settings(gd, angles)
    G, rep = dc.device_call(hip_ctx, b, mask, s)
    names = _lib.column_names(mask, s)
    bad = parity.compare_tables(G, po.oracle_featurize(b, mask, s), names, batch=b)
    assert not bad, "\n".join(bad[:20])
    n_live = 0
    for r in range(b.n_roi):
        e = gx.exact_glcm(b, r, s)
        assert e.degenerate or e.Ng == gd, (r, e.Ng)
        n_live += not e.degenerate
        bad += gx.compare_glcm_exact(G[r], e, e.Ng, names, len(angles), tag="roi %d: " % r)
    assert not bad, "\n".join(bad[:20])
    orders, flags = hip_ctx.roi_words(b.n_roi)
    print("matrix orders stated", orders, "of", n_live, "live ROIs; flags pending", flags)
    assert flags == 0 and orders <= n_live
