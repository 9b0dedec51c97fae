"""GPU test of the per-ROI binning slope of the compact co-occurrence builds (roi_features.hip: SLOPE1, s_stat[S_SLOPE], guard_flat).

One wave divides grey_depth / vmax out, publishes it through LDS, every wave bins its pixels with it and the degenerate guard takes its
two levels from it.  What can go wrong: a wave that reads the slot too early or a slot that phase 0 zeroes again (every level 1), a
quotient that differs from bin_pixel's in the last bit (a pixel on a level bound changes its level), a guard that fires for extrema
one level apart or sleeps for extrema in one level.  So: boxes of 17 x 20 px (340 px: beyond the wave-per-ROI kernel, on the
four-wave builds) and one 61 x 61 disk, whose pixels hold every level bound k vmax / Ng with the values one below and one above,
for pairs (vmin, vmax) on both sides of every form of the load pass and of the guard; masks 3 and 2 (the guard in the sums and in
the GLCM block), grey depths 8 and 16, one call under a non-zero soft_nan.  All columns are held to the oracle."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import device_call as dc
from tests import parity

pytestmark = pytest.mark.gpu

W, H = 17, 20
# (vmin, vmax): the rotated form (no zero, vmax < 2^15) | the zero form | the guard fires (extrema in one level) | extrema exactly one
# level apart at 8 levels (3072 -> 7) and at 16 levels (3584 -> 15) | both sides of vmax = 2^15 on a 16-bit table
PAIRS = [(1, 8), (1, 9), (7, 8), (8, 8), (1, 255), (1, 4095), (0, 255), (4094, 4095), (4095, 4095), (3072, 4095), (3584, 4095),
         (30000, 32767), (30000, 32768)]
# ... and with ranges beyond the 16-bit tables' launch (INTENSITY then runs a generic tier; GLCM alone stays on the compact build)
PAIRS_WIDE = [(1, 32767), (1, 32768)]


def _values(n, vmin, vmax, ng, rng):
    """n values in [vmin, vmax] that hold both extrema and every level bound k vmax / ng (rounded down and up) with its neighbours."""
    cand = {vmin, vmax}
    for k in range(ng + 1):
        lo = (k * vmax) // ng
        hi = -((-k * vmax) // ng)
        for b in (lo, hi):
            cand.update(v for v in (b - 1, b, b + 1) if vmin <= v <= vmax)
    v = np.array(sorted(cand), dtype=np.int64)
    assert len(v) <= n
    v = np.concatenate([v, rng.integers(vmin, vmax + 1, n - len(v))])
    rng.shuffle(v)
    return v.astype(np.uint32)


def _rois(pairs, with_disk, seed):
    rng = np.random.default_rng(seed)
    k = np.arange(W * H)
    rois = []
    for vmin, vmax in pairs:
        # (both depths' bounds in one ROI: 16 | 8, so the bounds of 8 levels are among those of 16)
        rois.append(dict(x=k // H, y=k % H, inten=_values(W * H, vmin, vmax, 16, rng)))
    if with_disk:
        yy, xx = np.mgrid[-30:31, -30:31]
        x, y = np.nonzero((xx * xx + yy * yy <= 900).T)                # column-major cloud order
        rois.append(dict(x=x, y=y, inten=_values(len(x), 1, 4095, 16, rng)))
    return rois


_cache = {}


def _case(name, gd, mask, soft_nan=0.0):
    """Batch, settings and the oracle's table: computed once, shared, never written to."""
    if name not in _cache:
        _cache[name] = _abi.batch_from_rois(_rois(PAIRS, True, 5) if name == "main" else _rois(PAIRS_WIDE, False, 6))
    b = _cache[name]
    s = _abi.default_settings(gd)
    s.soft_nan = soft_nan
    key = (name, gd, mask, soft_nan)
    if key not in _cache:
        _cache[key] = po.oracle_featurize(b, mask, s)
        _cache[key].setflags(write=False)
    return b, s, _cache[key]


def test_batch_holds_the_bounds_and_the_guard_cases():
    b = _abi.batch_from_rois(_rois(PAIRS, True, 5))
    assert list(zip(b.min_inten.tolist(), b.max_inten.tolist())) == PAIRS + [(1, 4095)]
    n = np.diff(b.px_offset)
    assert (n[:-1] == 340).all() and n[-1] == 2821 and b.bbox_w[0] == W and b.bbox_h[0] == H and b.bbox_w[-1] == 61
    v = b.inten[b.px_offset[5]:b.px_offset[6]].tolist()              # (1, 4095)
    for ng in (8, 16):
        for k in range(1, ng):
            assert {(k * 4095) // ng - 1, (k * 4095) // ng, (k * 4095) // ng + 1, (k * 4095) // ng + 2} <= set(v), (ng, k)
    lvl = lambda x, mx, ng: min(ng, int(np.floor(float(ng) / float(mx) * float(x) + 1.0)))
    assert lvl(3072, 4095, 8) == 7 and lvl(3584, 4095, 16) == 15 and lvl(4094, 4095, 8) == 8 and lvl(4094, 4095, 16) == 16


def _run(hip_ctx, name, gd, mask, monkeypatch, capfd, tier, soft_nan=0.0, stated=True):
    b, s, O = _case(name, gd, mask, soft_nan)
    monkeypatch.setenv("NYXHIP_DEBUG", "1")
    G, rep = dc.device_call(hip_ctx, b, mask, s, stated=stated)
    err = capfd.readouterr().err
    print("carve-outs", [l[3] for l in dc.launch_lines(err)])
    if tier:
        dc.assert_compact_tier(err, mask)
    names = _lib.column_names(mask, s)
    bad = parity.compare_tables(G, O, names, batch=b)
    assert not bad, "\n".join(bad[:20])
    return G, names, b


@pytest.mark.parametrize("gd", [8, 16])
@pytest.mark.parametrize("mask", [_abi.FAM_INTENSITY | _abi.FAM_GLCM, _abi.FAM_GLCM])
def test_level_bounds_and_guard(hip_ctx, mask, gd, monkeypatch, capfd):
    # (at 16 levels the disk's carve-out may exceed the eight-per-CU one: the seven-per-CU compact build shares the code under test)
    G, names, b = _run(hip_ctx, "main", gd, mask, monkeypatch, capfd, tier=gd == 8)
    j = names.index("GLCM_ASM_0")
    flat = [PAIRS.index(p) for p in ((8, 8), (4094, 4095), (4095, 4095))]
    assert (G[flat, j] == 0.0).all(), G[flat, j:j + 4]                 # the guard fires: the column is soft_nan = 0.0
    assert (G[PAIRS.index((3072 if gd == 8 else 3584, 4095)), j] != 0.0)  # one level apart: it does not


@pytest.mark.parametrize("gd", [8, 16])
@pytest.mark.parametrize("mask", [_abi.FAM_INTENSITY | _abi.FAM_GLCM, _abi.FAM_GLCM])
def test_both_sides_of_tiny_on_wide_ranges(hip_ctx, mask, gd, monkeypatch, capfd):
    _run(hip_ctx, "wide", gd, mask, monkeypatch, capfd, tier=(gd == 8 and mask == _abi.FAM_GLCM))


def test_through_the_classifier(hip_ctx, monkeypatch, capfd):
    _run(hip_ctx, "main", 8, _abi.FAM_INTENSITY | _abi.FAM_GLCM, monkeypatch, capfd, tier=True, stated=False)


def test_soft_nan(hip_ctx, monkeypatch, capfd):
    """(The GLCM row of a degenerate ROI is 0.0 under any soft_nan -- the oracle follows the reference's table there, glcm.cpp:27-95
    undone by save_value at :210-215.)"""
    G, names, b = _run(hip_ctx, "main", 8, _abi.FAM_INTENSITY | _abi.FAM_GLCM, monkeypatch, capfd, tier=True, soft_nan=-7.5)
    j = names.index("GLCM_ASM_0")
    assert G[PAIRS.index((4095, 4095)), j] == 0.0 and G[PAIRS.index((4094, 4095)), j] == 0.0
