"""GPU tests of the percentile code of roi_features.hip: the six percentiles come from six order statistics (the winning bin of
the reference's 100-bin histogram is min(99, idx100(x_c)), tests/test_percentile_shortcut_cpu.py) and the bounds of the winning bin and
its successor; the median's two order statistics come out of the same batched search.

Every ROI here lies in a box wider than 32 px, so the four-wave kernel serves it (every call of a cloud test reads that off
the launch report).  Rows are compared with the CPU oracle by the gates of tests/parity.py, where P01 .. P99, MEDIAN, MODE,
IQR, QCOD and ROBUST_MEAN are exact columns: no tolerance enters."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import parity, roi_assembly, synth

pytestmark = pytest.mark.gpu

INT = _abi.FAM_INTENSITY
INT_GLCM = _abi.FAM_INTENSITY | _abi.FAM_GLCM
CONFIGS = [(INT, 8), (INT_GLCM, 8), (INT_GLCM, 64)]
CONFIG_IDS = ["int-gd8", "int_glcm-gd8", "int_glcm-gd64"]
DBL_MAX = 1.7976931348623157e308
FAR = {2: 40, 3: 20, 4: 12, 5: 9}       # step that gives n diagonal pixels a box of 37 .. 41 px: beyond the 32 px of the smallest size class


def disk(r, rng, lo=1, hi=4096, const=None):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    y, x = np.nonzero(xx * xx + yy * yy <= r * r)
    o = np.lexsort((y, x))
    v = np.full(len(x), const, np.uint32) if const is not None else rng.integers(lo, hi, len(x)).astype(np.uint32)
    return dict(x=x[o], y=y[o], inten=v)


def box(w, h, inten):
    k = np.arange(w * h)
    return dict(x=k % w, y=k // w, inten=np.asarray(inten, np.uint32))


def valued(r, values, rng):
    """A disk of radius r whose pixels take `values` (a function n -> array) in a seeded random order."""
    d = disk(r, rng, const=0)
    return dict(d, inten=rng.permutation(np.asarray(values(len(d["x"])), np.uint32)))


def two_valued(R, share):
    def f(n):
        k = int(round(n * share))
        return np.concatenate([np.full(k, 5), np.full(n - k, 5 + R)])
    return f


def spanning(R, rng):
    """Random values in [5, 5 + R] with both ends present: the ROI's range is exactly R."""
    def f(n):
        v = rng.integers(5, 5 + R + 1, n)
        v[0], v[1] = 5, 5 + R
        return v
    return f


def diagonal(n, inten):
    k = np.arange(n) * FAR[n]
    return dict(x=k, y=k, inten=np.asarray(inten, np.uint32))


def build_groups():
    rng = np.random.default_rng(41)
    g = {}
    # integer cnt_p on a bin edge: 100 occupied bins of n / 100 pixels, cnt_p25 = runSum_25 -- bins 24 and 25 match, the last wins
    # (these three are symmetric about their mean: their skewness is rounding noise on either side, and parity's absolute allowance
    #  is 1e-12 of the column's scale -- the ordinary disk beside them gives the SKEWNESS column a scale)
    g["bin_edge"] = [box(40, 10, 1 + 10 * (np.arange(400) // 4)), box(50, 2, 1 + 10 * np.arange(100)), box(40, 5, 1 + 10 * (np.arange(200) // 2)),
                     disk(19, rng)]
    # empty bins around the winners
    g["two_valued"] = [valued(17, two_valued(R, share), rng) for R in (1, 2, 99, 100, 101, 4094, 16383) for share in (0.5, 0.05)]
    # the folded last bin: 60 % of the pixels at the maximum
    g["folded_last_bin"] = [valued(18, lambda n: np.where(np.arange(n) < (6 * n + 9) // 10, 1000, rng.integers(1, 1000, n)), rng)]
    # ranges with exact real boundaries (100, 200), the last range of the 16-bit tables, the first beyond them, a wide one
    g["exact_ranges"] = [valued(20, spanning(R, rng), rng) for R in (100, 200, 16383, 16384, 70000)]
    # few pixels on a far diagonal: distinct values, and values below 3 for ties
    g["few_pixels"] = [diagonal(n, 1 + 100 * rng.permutation(n)) for n in (2, 3, 4, 5)] + \
                      [diagonal(n, rng.integers(1, 3, n)) for n in (2, 3, 4, 5)] + [disk(20, rng, hi=70000)]
    # (the ordinary disk gives the columns that vanish on constant data a scale, as in the first group)
    g["constant"] = [disk(17, rng, const=7), disk(20, rng, const=0), disk(24, rng, const=4095), disk(19, rng)]
    g["ordinary"] = [disk(int(r), rng) for r in rng.integers(17, 32, 20)]
    return g


GROUPS = build_groups()
WIDE = disk(18, np.random.default_rng(43), hi=70000)     # range beyond the 16-bit tables, box of 37 px


def check(ctx, rois, mask, s):
    b = _abi.batch_from_rois(rois)
    G = ctx.featurize_host(b, mask, s)
    O = po.oracle_featurize(b, mask, s)
    bad = parity.compare_tables(G, O, _lib.column_names(mask, s), batch=b)
    assert not bad, "\n".join(bad[:20])
    return G


@pytest.mark.parametrize("mask,gd", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("group", list(GROUPS))
def test_group_matches_the_oracle(hip_ctx, group, mask, gd):
    """Each group with a wide-range disk beside it: the call then takes exact class lists, and the launch report shows that every ROI
    of the group ran in size class 1 -- the four-wave kernel -- and none in the wave-per-ROI kernel of the smallest class."""
    rois = GROUPS[group] + [WIDE]
    check(hip_ctx, rois, mask, _abi.default_settings(gd))
    rep = hip_ctx.launch_report()
    assert all(r["class"] >= 0 and r["size_class"] == 1 and r["workspace"] == 0 for r in rep), rep
    assert sum(r["rois"] for r in rep) == len(rois), rep


@pytest.mark.parametrize("mask,gd", CONFIGS, ids=CONFIG_IDS)
def test_every_roi_reaches_the_four_wave_kernel(hip_ctx, mask, gd):
    """All groups in one call.  The wide-range ROIs among them make the call take exact class lists; every ROI then sits in size
    class 1 (a box side of 33 .. 64 px, at most 4096 px) and runs from LDS -- none was served by the wave-per-ROI kernel of the
    smallest class."""
    rois = [r for grp in GROUPS.values() for r in grp]
    check(hip_ctx, rois, mask, _abi.default_settings(gd))
    rep = hip_ctx.launch_report()
    assert all(r["class"] >= 0 for r in rep), rep                                       # exact classes
    assert all(r["size_class"] == 1 for r in rep), rep
    assert sum(r["rois"] for r in rep) == len(rois), rep
    assert {r["wide_range"] for r in rep} == {0, 1}, rep                                # 16-bit tables and the sort engine
    assert all(r["workspace"] == 0 and r["cooperative"] == 0 for r in rep), rep


def test_tile_path_in_window_mode(hip_ctx):
    lab = synth.disk_label_tile(irregular=True, seed=12)
    it = synth.intensity_tile(12)
    lab[1000:1010, 960:1000] = 5000                          # the bin-edge ROI and a two-valued one among the disks
    it[1000:1010, 960:1000] = (1 + 10 * (np.arange(400) // 4)).reshape(10, 40)
    lab[980:990, 960:1000] = 5001
    it[980:990, 960:1000] = np.where(np.arange(400) % 20 == 0, 105, 5).reshape(10, 40)
    s = _abi.default_settings(8)
    labels, T = hip_ctx.featurize_tile_host(it, lab, INT_GLCM, s)
    b = roi_assembly.assemble(it, lab, DBL_MAX, -DBL_MAX)
    assert np.array_equal(labels, b.roi_label)
    bad = parity.compare_tables(T, po.oracle_featurize(b, INT_GLCM, s), _lib.column_names(INT_GLCM, s), batch=b)
    assert not bad, "\n".join(bad[:20])
