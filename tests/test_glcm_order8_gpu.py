"""GPU test of the fixed-order form of the 8-level GLCM feature launch (roi_features.hip: glcm_features_wave8<true>, taken by a wave
of glcm_features_kernel8 when the call has four angles and both of its ROIs have order 0 or 8).

The form reads the count matrix through wrapped indices (P[x][(x - l) & 7], P[x][(l - x) & 7]), joins the two halves of a |x - y|
diagonal through a lane's partner 8 - l (l = 4 is its own, l = 0 has none) and addresses the cell pass by constants.  A slip in any
of these moves single cells, so the cases put ONE occupied cell at every position of the matrix, for every angle:

  * 256 ROIs of four pixels: an adjacent pair at levels (r, c) laid out along the angle, one isolated pixel of 4095 and one of 1
    (they pin the extrema and have no neighbours).  Level r is the value (r - 1) * 512 + 256.  The matrix of the pair's angle has
    the one cell (r, c) -- ACOR = r c, CONTRAST = (r - c)^2, DIS = |r - c|, JMAX = 1 -- and the three other angles are blank;
  * the same 256 with a second, doubled pair at levels (2, 5) along the same angle: row and column marginals differ (one cell alone
    cannot tell a row from a column in the variance-class columns).

Both sets go through roi_small (four-pixel ROIs).  The workgroup kernel is the producer of a few random 17 x 20 boxes, of live / flat
ROIs in the pairings of tests/test_glcm_marginals_gpu.py and of an odd ROI count (the last wave holds one ROI).  A call with three
angles and a call at depth 7 run the general form in the same build.  No ROI with 32 768 pairs or more per angle (`big`:
sum_p >= 65536) is here: such a ROI has more than 32 768 pixels, and the dispatcher serves those from the global workspace, where
the GLCM columns close in the producer -- a 190 x 190 box with a symmetric matrix was tried under both masks and did not reach this
launch (profiles/r40_g8_order8.txt).

Depth 8, four angles, INTENSITY | GLCM and GLCM alone.  All columns are held to the oracle (tests/parity.py), the rational GLCM
columns also to tests/glcm_exact_ref.py under its own bound."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import device_call as dc
from tests import glcm_exact_ref as gx
from tests import parity

pytestmark = pytest.mark.gpu

ANGLES4 = (0, 45, 90, 135)
DXDY = {0: (1, 0), 45: (1, 1), 90: (0, 1), 135: (-1, 1)}      # neighbour = centre + (dx, dy); the matrix row is the centre's level
INT_GLCM = _abi.FAM_INTENSITY | _abi.FAM_GLCM
MASKS = (INT_GLCM, _abi.FAM_GLCM)


def _value(level):
    return (level - 1) * 512 + 256


def _cell_roi(r, c, angle, second):
    """Pair (centre r, neighbour c) along `angle` at rows 0-1, the extrema pixels at row 4, the doubled (2, 5) pair at rows 6-7 and 9-10:
    no two pixels of different groups touch, not even by a corner."""
    dx, dy = DXDY[angle]
    x, y, v = [2, 2 + dx, 0, 5], [0, dy, 4, 4], [_value(r), _value(c), 4095, 1]
    if second:
        for y0 in (6, 9):
            x += [2, 2 + dx]; y += [y0, y0 + dy]; v += [_value(2), _value(5)]
    return dict(x=np.array(x), y=np.array(y), inten=np.array(v, np.uint32))


def _settings(gd=8, angles=ANGLES4, symmetric=None):
    s = _abi.default_settings(gd)
    s.glcm_n_angles = len(angles)
    for i, a in enumerate(angles):
        s.glcm_angles[i] = a
    if symmetric is not None:
        s.glcm_symmetric = symmetric
    return s


_cache = {}


def _cells(second):
    key = ("cells", second)
    if key not in _cache:
        spec = [(r, c, a) for a in ANGLES4 for r in range(1, 9) for c in range(1, 9)]
        _cache[key] = (spec, _abi.batch_from_rois([_cell_roi(r, c, a, second) for r, c, a in spec]))
    return _cache[key]


def _exact(key, b, s):
    """exact_glcm of every ROI of a cached batch, once."""
    if ("exact", key) not in _cache:
        _cache[("exact", key)] = [gx.exact_glcm(b, r, s) for r in range(b.n_roi)]
    return _cache[("exact", key)]


def _oracle(key, b, mask, s):
    if ("oracle", key, mask) not in _cache:
        _cache[("oracle", key, mask)] = po.oracle_featurize(b, mask, s)
    return _cache[("oracle", key, mask)]


def _hold(hip_ctx, key, b, mask, s, order):
    G, rep = dc.device_call(hip_ctx, b, mask, s)
    names = _lib.column_names(mask, s)
    bad = parity.compare_tables(G, _oracle(key, b, mask, s), names, batch=b)
    assert not bad, "\n".join(bad[:20])
    for r, e in enumerate(_exact(key, b, s)):
        assert e.degenerate or e.Ng == order, (r, e.Ng)
        bad += gx.compare_glcm_exact(G[r], e, e.Ng, names, int(s.glcm_n_angles), tag="roi %d: " % r)
    assert not bad, "\n".join(bad[:20])
    return G, names, rep


@pytest.mark.parametrize("second", (False, True), ids=("one_cell", "second_pair"))
def test_cell_matrices_are_what_the_docstring_says(second):
    """CPU: the construction itself (no GPU call)."""
    spec, b = _cells(second)
    s = _settings()
    assert b.n_roi == 256 and (np.diff(b.px_offset) == (8 if second else 4)).all()
    assert (np.asarray(b.min_inten) == 1).all() and (np.asarray(b.max_inten) == 4095).all()
    for i, (r, c, a) in enumerate(spec):
        idx, I, _ = gx.levels_of(gx.dense_plane(b, i), 1, 4095, s)
        assert len(I) == 8
        for ang in ANGLES4:
            M = gx.cooc_matrix(idx, 8, *DXDY[ang], False)
            want = np.zeros((8, 8), np.int64)
            if ang == a:
                want[r - 1, c - 1] += 1
                if second:
                    want[1, 4] += 2
            assert (M == want).all(), (r, c, a, ang, M)


@pytest.mark.parametrize("mask", MASKS, ids=("int_glcm", "glcm"))
@pytest.mark.parametrize("second", (False, True), ids=("one_cell", "second_pair"))
def test_one_cell_at_every_position_and_angle(hip_ctx, mask, second):
    spec, b = _cells(second)
    s = _settings()
    G, names, _ = _hold(hip_ctx, ("cells", second), b, mask, s, 8)
    if second:
        return
    col = {n: j for j, n in enumerate(names)}
    for i, (r, c, a) in enumerate(spec):                       # the one cell, by its integers
        for ang in ANGLES4:
            want = (float(r * c), float((r - c) ** 2), float(abs(r - c)), 1.0) if ang == a else (float(s.soft_nan),) * 4
            got = tuple(G[i, col["GLCM_%s_%d" % (f, ang)]] for f in ("ACOR", "CONTRAST", "DIS", "JMAX"))
            assert got == want or (np.isnan(want[0]) and np.isnan(got).all()), (r, c, a, ang, got, want)


W, H = 17, 20
PATTERN = "LFFLLLFFLF"                                         # slots 2k and 2k + 1 share a wave: every pairing of live and flat, both orders


def _box(values):
    k = np.arange(W * H)
    return dict(x=k // H, y=k % H, inten=np.asarray(values, np.uint32))


def _boxes():
    if "boxes" not in _cache:
        rng = np.random.default_rng(408)
        rois = [_box(rng.integers(1, 4096, W * H)) if ch == "L" else _box(np.full(W * H, int(rng.integers(1, 4096)))) for ch in PATTERN]
        rois += [_box(rng.integers(1, 4096, W * H)) for _ in range(5)]        # random boxes; 15 ROIs: the last wave holds one
        _cache["boxes"] = _abi.batch_from_rois(rois)
    return _cache["boxes"]


def test_box_batch_shape():
    b = _boxes()
    assert b.n_roi % 2 == 1 and (np.diff(b.px_offset) > 256).all()            # the workgroup kernel is the producer
    flat = np.asarray(b.min_inten) == np.asarray(b.max_inten)
    assert "".join("F" if f else "L" for f in flat[:len(PATTERN)]) == PATTERN and not flat[len(PATTERN):].any()


@pytest.mark.parametrize("mask", MASKS, ids=("int_glcm", "glcm"))
def test_pairings_inside_a_wave(hip_ctx, mask):
    _hold(hip_ctx, "boxes", _boxes(), mask, _settings(), 8)


@pytest.mark.parametrize("gd,angles", ((8, (0, 45, 135)), (7, ANGLES4)), ids=("three_angles", "depth7"))
def test_general_form_beside_it(hip_ctx, gd, angles):
    b = _boxes()
    s = _settings(gd, angles)
    G, rep = dc.device_call(hip_ctx, b, INT_GLCM, s)
    names = _lib.column_names(INT_GLCM, s)
    bad = parity.compare_tables(G, po.oracle_featurize(b, INT_GLCM, s), names, batch=b)
    for r in range(b.n_roi):
        e = gx.exact_glcm(b, r, s)
        assert e.degenerate or e.Ng == gd
        bad += gx.compare_glcm_exact(G[r], e, e.Ng, names, len(angles), tag="roi %d: " % r)
    assert not bad, "\n".join(bad[:20])
