"""GPU tests of the robust statistics of roi_features.hip: in 16-bit-table launches ROBUST_MEAN, MEDIAN_ABSOLUTE_DEVIATION and
ROBUST_MEAN_ABSOLUTE_DEVIATION are read off the count and first-moment prefix tables at lox - 1, hix, kmed and t (the
identities: tests/test_robust_prefix_cpu.py).  Whole rows go against the CPU oracle through tests/parity.py.

Every ROI of two or more pixels lies in a 40 px wide box, so the four-wave kernel serves it and not the wave-per-ROI kernel of the
smallest size class (read off the launch report).  Two batches: ranges up to 4094 (a 4096-entry table: a word of first-moment
prefixes per 8 entries) and range 16383 (a 16384-entry table: coarser words).  `test_the_roi_set_covers_the_lookup_cases` states,
on the CPU, which positions of the lookups the set contains."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import parity, roi_assembly
from tests import robust_prefix_cases as rp

INT = _abi.FAM_INTENSITY
INT_GLCM = _abi.FAM_INTENSITY | _abi.FAM_GLCM
# INTENSITY alone and INTENSITY | GLCM at grey depth 8: the compact builds that defer the closing math; grey depth 100: a generic
# build that closes in the kernel
CONFIGS = [(INT, 8), (INT_GLCM, 8), (INT_GLCM, 100)]
CONFIG_IDS = ["int-gd8", "int_glcm-gd8", "int_glcm-gd100"]
DBL_MAX = 1.7976931348623157e308
SIZES = (1, 2, 3, 40, 97, 257, 600)
BOX_W = 40


def placed(values):
    """The values in reading order in a box 40 px wide; from two pixels on the last pixel of a short row sits in column 39."""
    v = np.asarray(values, np.uint32)
    k = np.arange(len(v))
    x, y = k % BOX_W, k // BOX_W
    if 2 <= len(v) < BOX_W:
        x[-1] = BOX_W - 1
    return dict(x=x, y=y, inten=v)


def build_groups():
    g = {"upto_4094": [], "r16383": []}
    for dist, R, v in rp.samples(SIZES, seed=11):
        g["r16383" if R == 16383 else "upto_4094"].append(v)
    return g


GROUPS = build_groups()


def wide_roi():
    """A range beyond the 16-bit tables in a box of 40 px: with it in the batch the call takes exact class lists."""
    rng = np.random.default_rng(43)
    return placed(rng.integers(1, 70000, 400))


def check(ctx, rois, mask, s, batch=None):
    b = batch if batch is not None else _abi.batch_from_rois(rois)
    G = ctx.featurize_host(b, mask, s)
    O = po.oracle_featurize(b, mask, s)
    bad = parity.compare_tables(G, O, _lib.column_names(mask, s), batch=b)
    assert not bad, "\n".join(bad[:20])


def test_the_roi_set_covers_the_lookup_cases():
    """CPU only: the positions the lookups of the set's ROIs take (robust_prefix_cases.points restates the kernel's derivation)."""
    got = set()
    for v in GROUPS["upto_4094"] + GROUPS["r16383"]:
        p = rp.points(v)
        if p["n"] == 1:
            got.add("n = 1")
            continue                                  # (the smallest size class: the wave-per-ROI kernel, unless the box says otherwise)
        if p["n"] == 2:
            got.add("n = 2")
        for q in p["lookups"]:
            if q % 8 == 0:
                got.add("point = 0 (mod 8)")
            if q % 8 == 7:
                got.add("point = 7 (mod 8)")
            for edge in (p["Q"], 2 * p["Q"], 3 * p["Q"]):      # first entries of the second .. fourth wave's quarter of the table
                if edge <= p["R"] and q == edge - 1:
                    got.add("point = Q - 1")
                if edge <= p["R"] and q == edge:
                    got.add("point = Q")
        if p["empty"]:
            got.add("empty range")
        else:
            if p["lox"] == 0:
                got.add("lox = 0")
            if p["hix"] == p["R"]:
                got.add("hix = range")
            if p["K"] == 0:
                got.add("K = 0")
            if p["K"] == 1:
                got.add("K = 1")
            if p["K"] == p["n"]:
                got.add("K = n")
        if p["half"]:
            got.add("half-integer median")
        if p["R"] >= 2048:
            got.add("two engine steps per wave")
        if p["R"] == 16383:
            got.add("range 16383")
    want = {"point = 0 (mod 8)", "point = 7 (mod 8)", "point = Q - 1", "point = Q", "lox = 0", "hix = range", "K = 1", "K = n",
            "half-integer median", "n = 1", "n = 2", "two engine steps per wave", "range 16383", "empty range", "K = 0"}
    assert want <= got, sorted(want - got)


@pytest.mark.gpu
@pytest.mark.parametrize("mask,gd", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("group", list(GROUPS))
def test_rows_match_the_oracle(hip_ctx, group, mask, gd):
    rois = [placed(v) for v in GROUPS[group]] + [wide_roi()]
    check(hip_ctx, rois, mask, _abi.default_settings(gd))
    rep = hip_ctx.launch_report()
    assert all(r["class"] >= 0 and r["workspace"] == 0 for r in rep), rep                  # exact classes, from LDS
    assert sum(r["rois"] for r in rep) == len(rois), rep
    single = sum(1 for v in GROUPS[group] if len(v) == 1)
    assert sum(r["rois"] for r in rep if r["size_class"] == 0) == single, rep               # everything else: the four-wave kernel
    assert all(r["size_class"] <= 1 for r in rep), rep


@pytest.mark.gpu
def test_one_pixel_rois_in_the_four_wave_kernel(hip_ctx):
    """INTENSITY reads no box: stating a 40 px wide one for the one- and two-pixel ROIs sends them to the four-wave kernel."""
    rng = np.random.default_rng(5)
    rois = [placed([7]), placed([4094 + rp.BASE]), placed([9, 9]), placed([5, 16388]), placed(rp.sample("uniform", 511, 97, rng)), wide_roi()]
    b = _abi.batch_from_rois(rois)
    b.bbox_w[:] = BOX_W
    check(hip_ctx, rois, INT, _abi.default_settings(8), batch=b)
    rep = hip_ctx.launch_report()
    assert all(r["class"] >= 0 and r["size_class"] == 1 and r["workspace"] == 0 for r in rep), rep
    assert sum(r["rois"] for r in rep) == len(rois), rep


@pytest.mark.gpu
def test_tile_path_in_window_mode(hip_ctx):
    """Every third ROI of the set (two pixels and more) in the cells of a 256 x 256 tile, through the fused tile path."""
    cases = [v for v in GROUPS["upto_4094"] + GROUPS["r16383"] if len(v) >= 2][::3]
    assert len(cases) == 84 and any(int(v.max() - v.min()) == 16383 for v in cases)      # 6 x 14 cells of 42 x 16 px
    it = np.zeros((256, 256), np.uint32)
    lab = np.zeros((256, 256), np.uint32)
    for k, v in enumerate(cases):
        r = placed(v)
        x0, y0 = (k % 6) * 42, (k // 6) * 16
        it[y0 + r["y"], x0 + r["x"]] = r["inten"]
        lab[y0 + r["y"], x0 + r["x"]] = k + 1
    s = _abi.default_settings(8)
    labels, T = hip_ctx.featurize_tile_host(it, lab, INT_GLCM, s)
    b = roi_assembly.assemble(it, lab, DBL_MAX, -DBL_MAX)
    assert np.array_equal(labels, b.roi_label) and len(labels) == len(cases)
    bad = parity.compare_tables(T, po.oracle_featurize(b, INT_GLCM, s), _lib.column_names(INT_GLCM, s), batch=b)
    assert not bad, "\n".join(bad[:20])
