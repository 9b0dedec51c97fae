"""Feret, Martin and Nassenstein diameters on the GPU: the HIP rows against values recorded from the reference's own classes
(tests/golden/caliper), against tests/caliper_ref.py on other inputs, and against themselves across every way a row can be
requested.  The two angles and the three modes are compared exactly, every other column at parity.REL_TOL; bit equality is what
the construction aims at: against the restatement (pinned to the reference's per-angle diameters bit for bit) it is asserted, on the
inputs of `wide` and on other seeds; against the recorded tables every test prints how far from it the rows are."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import caliper_cases, caliper_ref, parity, radial_cases, synth
from tests.test_caliper_cpu import mismatches

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FE, MA, NA = _abi.FAM_FERET, _abi.FAM_MARTIN, _abi.FAM_NASSENSTEIN
CAL = FE | MA | NA
OUTLINE = _abi.FAM_FRACTAL | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS
GOLD = caliper_cases.golden()


def caliper_of(ctx, b, mask, s):
    """(the caliper columns present in `mask`, their names, the other columns, their names) of one call."""
    names = _lib.column_names(mask, s)
    T = ctx.featurize_host(b, mask, s)
    idx = [i for i, n in enumerate(names) if n in caliper_ref.NAMES]
    rest = [i for i in range(len(names)) if i not in set(idx)]
    return T[:, idx], [names[i] for i in idx], T[:, rest], [names[i] for i in rest]


def same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def report(tag, got, want):
    d = np.abs(got - want)
    print(f"{tag}: {len(got)} ROIs; bit-identical values {(got == want).mean():.4f}; largest difference per column {d.max(0)}")


@pytest.mark.parametrize("name", list(caliper_cases.CASES))
def test_hip_rows_match_the_reference_classes(hip_ctx, name):
    b = caliper_cases.batch(name)
    want = GOLD[name]["table"]
    s = _abi.default_settings(64)
    got = hip_ctx.featurize_host(b, CAL, s)
    report(name, got, want)
    bad = mismatches(got, want)
    assert not bad, "\n".join(bad[:10])


def test_degenerate_rows_under_a_non_zero_soft_nan(hip_ctx):
    b = caliper_cases.batch("degenerate")
    s = _abi.default_settings(64)
    s.soft_nan = -7.5
    got = hip_ctx.featurize_host(b, CAL, s)
    assert (got[0] == -7.5).all()
    assert not mismatches(got, GOLD["degenerate_softnan"]["table"])
    for fam, sl in ((FE, slice(0, 8)), (MA, slice(8, 14)), (NA, slice(14, 20))):
        assert same(hip_ctx.featurize_host(b, fam, s), got[:, sl])


def test_placed_through_the_origin_entry_and_without_it(hip_ctx):
    b = caliper_cases.batch("placed")
    s = _abi.default_settings(64)
    got = hip_ctx.featurize_host(b, CAL, s)                                  # nyxhip_featurize_batch_at
    report("placed", got, GOLD["placed"]["table"])
    assert not mismatches(got, GOLD["placed"]["table"])
    assert (got[:8] != got[8:16]).any()                                     # the origin is read
    plain = _abi.HostBatch(b.roi_label, b.px_offset, b.x, b.y, b.inten, b.bbox_w, b.bbox_h, b.min_inten, b.max_inten)
    old = hip_ctx.featurize_host(plain, CAL, s)                             # nyxhip_featurize_batch: every origin (0, 0)
    assert same(old[:8], got[:8]) and same(old[8:16], got[:8]) and same(old[16:], got[:8])
    # no other family reads the origin
    m = OUTLINE | _abi.FAM_INTENSITY | _abi.FAM_GLCM | _abi.FAM_RADIAL
    assert same(hip_ctx.featurize_host(plain, m, s), hip_ctx.featurize_host(b, m, s))


def test_rows_do_not_depend_on_the_companions(hip_ctx):
    """Each bit alone, pairs, all three; beside the outline bits, the contour families, INTENSITY | GLCM (the moved column bases and
    the zeroed span) and every family: the same bits, and the other columns are those of the call without the caliper bits."""
    # (the discs of radius 33 and 70 are of the size classes whose texture / Gabor / large-ROI launches carry column bases of their own)
    big = dict(radial_cases._mask_roi(radial_cases.disc(70), 77))
    big["x"], big["y"] = big["x"] + 500, big["y"] + 900
    b = _abi.batch_from_rois(caliper_cases.degenerate() + caliper_cases.shapes()[:14] + caliper_cases.placed()[8:12] + [big])
    s = _abi.default_settings(64)
    all20 = hip_ctx.featurize_host(b, CAL, s)
    col = {n: all20[:, i] for i, n in enumerate(caliper_ref.NAMES)}
    for fam in (FE, MA, NA, FE | MA, MA | NA, FE | NA):
        got, names, _, _ = caliper_of(hip_ctx, b, fam, s)
        assert all(same(got[:, i], col[n]) for i, n in enumerate(names)), fam
    extras = [OUTLINE, _abi.FAM_EULER, _abi.FAM_SMOMS | _abi.FAM_IMOMS | _abi.FAM_RADIAL, _abi.FAM_INTENSITY | _abi.FAM_GLCM, _abi.FAM_GLCM,
              _abi.FAM_ALL, _abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE]
    for extra in extras:
        for fam in (CAL, MA, FE, NA, FE | NA):              # (each moves col_martin / col_nassenstein / col_euler differently)
            got, names, rest, rest_names = caliper_of(hip_ctx, b, fam | extra, s)
            assert all(same(got[:, i], col[n]) for i, n in enumerate(names)), (fam, extra)
            assert rest_names == _lib.column_names(extra, s)
            plain = hip_ctx.featurize_host(b, extra, s)
            assert same(plain, rest), (fam, extra, np.argwhere(~((plain == rest) | (np.isnan(plain) & np.isnan(rest))))[:5])


def test_other_inputs_and_permuted_pixel_orders(hip_ctx):
    rois = synth.random_rois(20, seed=79, rmax=25) + [radial_cases._mask_roi(radial_cases.disc(k), 100 + k) for k in (2, 17)]
    rois = [dict(r, x=r["x"] + 977 * i, y=r["y"] + 3301 * i) for i, r in enumerate(rois)]
    b = _abi.batch_from_rois(rois)
    s = _abi.default_settings(64)
    want = caliper_ref.table(b)
    got = hip_ctx.featurize_host(b, CAL, s)
    report("seed 79", got, want)
    assert not mismatches(got, want)
    # the restatement is pinned to the reference's per-angle diameters bit for bit, and the kernel runs the same fp64 operations
    # with the host's sin / cos: every value equal, not merely close
    assert same(got, want), np.argwhere(got != want)[:5]
    rng = np.random.default_rng(6)
    for r in rois:
        p = rng.permutation(len(r["x"]))
        r["x"], r["y"], r["inten"] = r["x"][p], r["y"][p], r["inten"][p]
    perm = hip_ctx.featurize_host(_abi.batch_from_rois(rois), CAL, s)
    assert same(perm, got), np.argwhere(perm != got)[:5]


def test_wide_boxes_on_both_sides_of_the_lds_limit(hip_ctx):
    """The same shapes just below the LDS column table (LDS path), and just above it (global tables, alone and in one batch with the
    others): the rows of the restatement, and the same bits whichever path served an ROI."""
    rois = caliper_cases.wide()
    s = _abi.default_settings(64)
    b = _abi.batch_from_rois(rois)
    want = caliper_ref.table(b)
    got = hip_ctx.featurize_host(b, CAL, s)                                  # mixed: a deferring launch and a list launch
    report("wide", got, want)
    assert not mismatches(got, want)
    assert same(got, want), np.argwhere(got != want)[:5]                    # the same bits as the restatement on both paths
    below = hip_ctx.featurize_host(_abi.batch_from_rois(rois[:6]), CAL, s)   # every box within the table: one LDS launch
    assert same(below, got[:6])
    above = hip_ctx.featurize_host(_abi.batch_from_rois(rois[6:]), CAL, s)
    assert same(above, got[6:])


def test_tile_path_and_device_budget(hip_ctx):
    """The fused tile path hands the kernel the box origins inside the tile: the rows of the batch path with origins, bit for bit; a
    2 MiB device budget over five stacked tiles returns the single-chunk result."""
    it, lab = radial_cases.tile()
    b = caliper_cases.batch("tile")
    s = _abi.default_settings(64)
    alone = hip_ctx.featurize_host(b, CAL, s)
    labels, T = hip_ctx.featurize_tile_host(it, lab, CAL, s)
    assert list(labels) == list(b.roi_label) and same(T, alone)
    assert not mismatches(T, GOLD["tile"]["table"])
    mask = CAL | OUTLINE | _abi.FAM_INTENSITY | _abi.FAM_GLCM | _abi.FAM_SMOMS
    names = _lib.column_names(mask, s)
    I, M = np.stack([it] * 5), np.stack([lab] * 5)
    one = hip_ctx.featurize_tiles_host(I, M, mask, s, max_device_bytes=1 << 34)
    many = hip_ctx.featurize_tiles_host(I, M, mask, s, max_device_bytes=2 << 20)
    assert (one[0] == many[0]).all() and (one[1] == many[1]).all() and same(one[2], many[2])
    idx = [i for i, n in enumerate(names) if n in caliper_ref.NAMES]
    assert same(many[2][:, idx], np.tile(alone, (5, 1)))
    plain = hip_ctx.featurize_tiles_host(I, M, mask & ~CAL, s, max_device_bytes=2 << 20)
    rest = [i for i in range(len(names)) if i not in set(idx)]
    assert same(plain[2], many[2][:, rest])


def test_through_nyxus_featurize():
    api = json.load(open(os.path.join(ROOT, "tests", "golden", "caliper", "api_expected.json")))
    it, lab = radial_cases.tile()
    for case in api["cases"].values():
        nyx = nyxus_amd.Nyxus(case["features"])
        df = nyx.featurize(it.astype(api["inten_dtype"]), lab)
        assert list(df.columns[-len(case["columns"]):]) == case["columns"]
        assert list(df["ROI_label"]) == api["labels"]
        got = df[case["columns"]].values.astype(float)
        want = np.array(case["numeric"])
        full_g, full_w = np.zeros((len(got), 20)), np.zeros((len(got), 20))
        for j, c in enumerate(case["columns"]):
            full_g[:, caliper_ref.NAMES.index(c)], full_w[:, caliper_ref.NAMES.index(c)] = got[:, j], want[:, j]
        bad = mismatches(full_g, full_w)
        assert not bad, "\n".join(bad[:10])
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["CONVEX_HULL_AREA"])


def test_unassigned_bits_are_still_bad_masks(hip_ctx):
    b = caliper_cases.batch("degenerate")
    for bit in (12, 14, 31):
        with pytest.raises(_lib.NyxHipError) as ei:
            hip_ctx.featurize_host(b, CAL | (1 << bit), _abi.default_settings(8))
        assert ei.value.code == 1
