"""GPU tests of the deferred intensity closing (roi_features.hip: the 64-VGPR builds leave the single-lane output math of the
intensity block to intensity_close_kernel, a lane per ROI behind the feature launch).

Which ROIs defer is decided per ROI and per launch: blank ROIs, the smallest size class (roi_small.hip), wide ranges and every ROI
beyond size class 1 close where they always did, so a call mixes both kinds.  Every case checks rows against the CPU oracle with the
gates of tests/parity.py; the last two pin that nothing is carried from call to call and that a row does not depend on its companions."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import parity, roi_assembly, synth

pytestmark = pytest.mark.gpu

INT = _abi.FAM_INTENSITY
INT_GLCM = _abi.FAM_INTENSITY | _abi.FAM_GLCM
DBL_MAX = 1.7976931348623157e308


def disk(r, rng, lo=1, hi=4096, const=None):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    y, x = np.nonzero(xx * xx + yy * yy <= r * r)
    o = np.lexsort((y, x))
    v = np.full(len(x), const, np.uint32) if const is not None else rng.integers(lo, hi, len(x)).astype(np.uint32)
    return dict(x=x[o], y=y[o], inten=v)


FAR = {2: 40, 3: 20, 4: 12, 5: 9}       # step that gives n diagonal pixels a box of 37 .. 41 px: beyond the 32 px of the smallest size class


def points(n, step, rng, hi=4096):
    """n pixels on a diagonal, `step` apart: step 1 stays in the smallest size class (roi_small.hip closes it), FAR[n] leaves it by
    the box alone, so the four-wave kernel serves the ROI and -- in its 64-VGPR builds -- defers the closing."""
    k = np.arange(n)
    return dict(x=k * step, y=k * step, inten=rng.integers(1, hi, n).astype(np.uint32))


def edge_rois(seed=3):
    """Blank, constant, single-pixel and n = 2 .. 5 ROIs (the dn > 1 guards of the variances, the n > 3 / n > 4 guards of skewness
    and kurtosis).  n = 2 .. 5 appear both inside the smallest size class and -- by a box beyond 32 px -- outside it; a single pixel
    has a 1 x 1 box and cannot leave the smallest class, so n = 1 never reaches the closing launch.  Ordinary disks between."""
    rng = np.random.default_rng(seed)
    rois = [disk(20, rng), disk(14, rng, const=0), disk(3, rng, const=0), disk(14, rng, const=7), disk(3, rng, const=7),
            dict(x=[0], y=[0], inten=[9]), dict(x=[5], y=[2], inten=[0])]
    for n in (2, 3, 4, 5):
        rois.append(points(n, 1, rng))
        rois.append(points(n, FAR[n], rng))
        rois.append(points(n, FAR[n], rng, hi=3))            # few distinct values: ties in median and mode
        rois.append(dict(points(n, FAR[n], rng), inten=np.full(n, 5, np.uint32)))   # constant: zero variance on the deferred path
    rois += [disk(25, rng, lo=0, hi=300), disk(30, rng), disk(9, rng), disk(18, rng, lo=0, hi=2)]
    return rois


def with_slide(rois, lo=3.0, hi=60000.0):
    return [dict(r, slide_min=lo, slide_max=hi) for r in rois]


def check(ctx, rois, mask, s):
    b = _abi.batch_from_rois(rois)
    G = ctx.featurize_host(b, mask, s)
    O = po.oracle_featurize(b, mask, s)
    bad = parity.compare_tables(G, O, _lib.column_names(mask, s), batch=b)
    assert not bad, "\n".join(bad[:20])
    return G


def same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("mask", [INT, INT_GLCM])
@pytest.mark.parametrize("slide", [False, True])
@pytest.mark.parametrize("soft_nan", [0.0, -7.5])
def test_edge_rois_match_the_oracle(hip_ctx, mask, slide, soft_nan):
    """(At soft_nan = -7.5 the GLCM row of a blank or constant ROI is 0.0, not soft_nan: the oracle follows the reference's table there,
    glcm.cpp:27-95 undone by save_value at :210-215 -- tests/test_soft_nan_cpu.py.)"""
    s = _abi.default_settings(8)
    s.soft_nan = soft_nan
    rois = edge_rois()
    check(hip_ctx, with_slide(rois) if slide else rois, mask, s)


@pytest.mark.parametrize("mask", [INT, INT_GLCM])
def test_few_pixel_rois_reach_the_four_wave_kernel(hip_ctx, mask):
    """n = 2 .. 5 pixels in boxes beyond 32 px, against the oracle, in a call whose launch report shows where they ran: the wide-range
    companion makes the call take exact class lists, and the list of size class 1 (16-bit tables) then holds exactly these ROIs --
    none of them was served by the wave-per-ROI kernel of the smallest class."""
    rng = np.random.default_rng(17)
    few = []
    for n in (2, 3, 4, 5):
        few += [points(n, FAR[n], rng), points(n, FAR[n], rng, hi=3), dict(points(n, FAR[n], rng), inten=np.full(n, 5, np.uint32)),
                dict(points(n, FAR[n], rng), inten=np.arange(1, n + 1, dtype=np.uint32) * 100)]
    s = _abi.default_settings(8)
    check(hip_ctx, few + [disk(12, rng, hi=70000)], mask, s)
    rep = hip_ctx.launch_report()
    assert all(r["class"] >= 0 for r in rep), rep                                       # exact classes
    assert [r["rois"] for r in rep if r["size_class"] == 1 and r["wide_range"] == 0] == [len(few)], rep
    assert not [r for r in rep if r["size_class"] == 0 and r["wide_range"] == 0], rep   # nobody in the smallest 16-bit class
    assert all(r["workspace"] == 0 and r["cooperative"] == 0 for r in rep if r["size_class"] == 1), rep


@pytest.mark.parametrize("mask,gd", [(INT, 8), (INT_GLCM, 8), (INT_GLCM, 64)])
def test_mixed_sizes_in_several_launch_groups(hip_ctx, mask, gd):
    """Small-class, mid-class, large-class and wide-range ROIs in one call: deferred and in-kernel closings side by side."""
    rng = np.random.default_rng(8)
    rois = edge_rois(5) + [disk(int(r), rng) for r in rng.integers(2, 32, 40)]
    rois += [disk(50, rng), disk(100, rng), disk(170, rng), disk(12, rng, hi=70000), disk(20, rng, hi=200000), disk(28, rng, const=0)]
    rois = [rois[i] for i in rng.permutation(len(rois))]
    s = _abi.default_settings(gd)
    check(hip_ctx, rois, mask, s)
    rep = hip_ctx.launch_report()
    assert len(rep) >= 4, rep                                # several launch groups


@pytest.mark.parametrize("mask", [INT, INT_GLCM])
def test_tile_path_in_window_mode(hip_ctx, mask):
    lab = synth.disk_label_tile(irregular=True, seed=9)
    lab[1000:1020, 1000:1020] = 5000                         # a blank ROI and a constant one among the disks
    lab[980:990, 1000:1020] = 5001
    it = synth.intensity_tile(9)
    it[1000:1020, 1000:1020] = 0
    it[980:990, 1000:1020] = 11
    s = _abi.default_settings(8)
    labels, T = hip_ctx.featurize_tile_host(it, lab, mask, s)
    b = roi_assembly.assemble(it, lab, DBL_MAX, -DBL_MAX)
    assert np.array_equal(labels, b.roi_label)
    bad = parity.compare_tables(T, po.oracle_featurize(b, mask, s), _lib.column_names(mask, s), batch=b)
    assert not bad, "\n".join(bad[:20])


def test_consecutive_calls_share_no_state(hip_ctx):
    """Two calls on one context with different ROI counts, orders and output tables: a flag or a record left by the first call would
    show in the second (ROI i of the second call is a different ROI, blank or of another class, where the first one deferred)."""
    rng = np.random.default_rng(21)
    s = _abi.default_settings(8)
    first = [disk(int(r), rng) for r in rng.integers(17, 31, 64)]
    G1 = check(hip_ctx, first, INT_GLCM, s)
    second = [disk(14, rng, const=0), disk(3, rng), disk(90, rng), disk(20, rng, hi=100000)] * 4 + [disk(22, rng) for _ in range(7)]
    G2 = check(hip_ctx, second, INT_GLCM, s)
    assert G1.shape[0] != G2.shape[0]
    check(hip_ctx, second[:9], INT, s)                       # ... and another mask, fewer ROIs, on the same context
    again = hip_ctx.featurize_host(_abi.batch_from_rois(first), INT_GLCM, s)
    assert same(G1, again).all()


@pytest.mark.parametrize("mask", [INT, INT_GLCM])
def test_a_row_alone_and_among_companions(hip_ctx, mask):
    rng = np.random.default_rng(33)
    s = _abi.default_settings(8)
    mine = [disk(24, rng), points(4, FAR[4], rng), points(2, FAR[2], rng), disk(17, rng, lo=0, hi=40), disk(30, rng, const=3)]
    others = [disk(110, rng), disk(5, rng), disk(19, rng, const=0), disk(15, rng, hi=90000), disk(29, rng)]
    together = hip_ctx.featurize_host(_abi.batch_from_rois(others[:3] + mine + others[3:]), mask, s)[3:3 + len(mine)]
    for k, r in enumerate(mine):
        alone = hip_ctx.featurize_host(_abi.batch_from_rois([r]), mask, s)
        assert same(alone[0], together[k]).all(), (k, np.nonzero(~same(alone[0], together[k])))
