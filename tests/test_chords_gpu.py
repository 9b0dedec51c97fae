"""MAXCHORDS_* / ALLCHORDS_* on the GPU: the HIP rows against values recorded from the reference's own ChordsFeature
(tests/golden/chords), against tests/chords_ref.py on other inputs, and against themselves across every way a row can be requested.
MAX, MIN, MEDIAN, MODE and the four angles are compared exactly, MEAN and STDDEV at parity.REL_TOL; the kernel closes Welford's sums on
one lane in insertion order, so bit equality with the restatement (pinned to the reference bit for bit) is asserted as well."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import chords_cases, chords_ref, radial_cases, synth
from tests.test_chords_cpu import mismatches

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = _abi.FAM_CHORDS
CAL = _abi.FAM_FERET | _abi.FAM_MARTIN | _abi.FAM_NASSENSTEIN
OUTLINE = _abi.FAM_FRACTAL | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS
GOLD = chords_cases.golden()


def chords_of(ctx, b, mask, s):
    """(the chords columns, the other columns, their names) of one call."""
    names = _lib.column_names(mask, s)
    T = ctx.featurize_host(b, mask, s)
    idx = [i for i, n in enumerate(names) if n in chords_ref.NAMES]
    rest = [i for i in range(len(names)) if i not in set(idx)]
    assert [names[i] for i in idx] == chords_ref.NAMES
    return T[:, idx], T[:, rest], [names[i] for i in rest]


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def report(tag, got, want):
    print(f"{tag}: {len(got)} ROIs; bit-identical values {(got == want).mean():.4f}; largest difference per column {np.abs(got - want).max(0)}")


@pytest.mark.parametrize("name", list(chords_cases.CASES))
def test_hip_rows_match_the_reference_class(hip_ctx, name):
    b = chords_cases.batch(name)
    want = GOLD[name]["table"]
    got = hip_ctx.featurize_host(b, CH, _abi.default_settings(64))
    assert got.shape == want.shape                                           # no ROI is left out
    report(name, got, want)
    bad = mismatches(got, want)
    assert not bad, "\n".join(bad[:10])
    assert same(got, want), np.argwhere(got != want)[:5]                    # sequential closing: the reference's bits


def test_rows_under_a_non_zero_soft_nan(hip_ctx):
    s = _abi.default_settings(64)
    s.soft_nan = -7.5
    for name, key in (("degenerate", "degenerate_softnan"), ("zeros", "zeros")):
        got = hip_ctx.featurize_host(chords_cases.batch(name), CH, s)
        assert not mismatches(got, GOLD[key]["table"]) and same(got, GOLD[key]["table"])
    assert (hip_ctx.featurize_host(chords_cases.batch("degenerate"), CH, s)[:2] == 0).all()   # zeros, not soft_nan (chords.cpp:59-60)


def test_placed_through_the_origin_entry_and_without_it(hip_ctx):
    b = chords_cases.batch("placed")
    s = _abi.default_settings(64)
    got = hip_ctx.featurize_host(b, CH, s)                                   # nyxhip_featurize_batch_at
    assert (got[:8] != got[8:16]).any() and (got[:8] != got[16:]).any()     # the origin is read
    plain = _abi.HostBatch(b.roi_label, b.px_offset, b.x, b.y, b.inten, b.bbox_w, b.bbox_h, b.min_inten, b.max_inten)
    old = hip_ctx.featurize_host(plain, CH, s)                              # nyxhip_featurize_batch: every origin (0, 0)
    assert same(old[:8], got[:8]) and same(old[8:16], got[:8]) and same(old[16:], got[:8])


def test_rows_do_not_depend_on_the_companions(hip_ctx):
    """Beside the caliper bits, the outline bits, the contour families, INTENSITY | GLCM (the moved column bases and the zeroed span)
    and every family: the same bits, and the other columns are those of the call without bit 21."""
    big = dict(radial_cases._mask_roi(radial_cases.disc(70), 77))
    big["x"], big["y"] = big["x"] + 500, big["y"] + 900
    b = _abi.batch_from_rois(chords_cases.degenerate() + chords_cases.shapes()[:14] + chords_cases.zeros() + chords_cases.placed()[8:12] + [big])
    s = _abi.default_settings(64)
    alone = hip_ctx.featurize_host(b, CH, s)
    assert same(alone, chords_ref.table(b))
    extras = [CAL, _abi.FAM_NASSENSTEIN | _abi.FAM_EULER, OUTLINE, _abi.FAM_SMOMS | _abi.FAM_IMOMS | _abi.FAM_RADIAL, _abi.FAM_INTENSITY | _abi.FAM_GLCM,
              _abi.FAM_GLCM, _abi.FAM_ALL, _abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE | CAL]
    for extra in extras:
        got, rest, rest_names = chords_of(hip_ctx, b, CH | extra, s)
        assert same(got, alone), (extra, np.argwhere(got != alone)[:5])
        assert rest_names == _lib.column_names(extra, s)
        plain = hip_ctx.featurize_host(b, extra, s)
        assert same(plain, rest), (extra, np.argwhere(~((plain == rest) | (np.isnan(plain) & np.isnan(rest))))[:5])
    # a row is the same whatever else shares its call
    for r in (0, 9, 21, 24, len(alone) - 1):
        sub = _abi.batch_from_rois((chords_cases.degenerate() + chords_cases.shapes()[:14] + chords_cases.zeros() + chords_cases.placed()[8:12] + [big])[r:r + 1])
        assert same(hip_ctx.featurize_host(sub, CH, s), alone[r:r + 1]), r


def test_other_inputs_and_permuted_pixel_orders(hip_ctx):
    rois = synth.random_rois(20, seed=83, rmax=25, value_modes=(4096, 256, 65536)) + [radial_cases._mask_roi(radial_cases.disc(k), 100 + k) for k in (2, 17)]
    rois = [dict(r, x=r["x"] + 977 * i, y=r["y"] + 3301 * i) for i, r in enumerate(rois)]
    b = _abi.batch_from_rois(rois)
    s = _abi.default_settings(64)
    want = chords_ref.table(b)
    got = hip_ctx.featurize_host(b, CH, s)
    report("seed 83", got, want)
    assert not mismatches(got, want)
    assert same(got, want), np.argwhere(got != want)[:5]
    # ROIs without zero-intensity pixels: no cell depends on which of its pixels came last
    keep = [i for i, r in enumerate(rois) if (r["inten"] != 0).all()]
    assert len(keep) >= 10
    rng = np.random.default_rng(6)
    perm = []
    for i in keep:
        r = rois[i]
        p = rng.permutation(len(r["x"]))
        perm.append(dict(r, x=r["x"][p], y=r["y"][p], inten=r["inten"][p]))
    out = hip_ctx.featurize_host(_abi.batch_from_rois(perm), CH, s)
    assert same(out, got[keep]), np.argwhere(out != got[keep])[:5]


def test_both_sides_of_the_lds_limit(hip_ctx):
    """Thin shapes just below the LDS bit plane and just above it (global planes), alone and in one batch: the recorded rows, and the
    same bits whichever path served an ROI."""
    rois = chords_cases.limit()
    s = _abi.default_settings(64)
    got = hip_ctx.featurize_host(_abi.batch_from_rois(rois), CH, s)          # mixed: the LDS launch and the list launch
    assert same(got, GOLD["limit"]["table"])
    assert same(hip_ctx.featurize_host(_abi.batch_from_rois(rois[:6]), CH, s), got[:6])     # nothing listed
    assert same(hip_ctx.featurize_host(_abi.batch_from_rois(rois[6:]), CH, s), got[6:])     # everything listed
    # the same ROI through the LDS plane and -- with one zero-intensity pixel on a cell it shares with nobody -- through global planes
    r = dict(chords_cases.shapes()[4])                                       # the disc of radius 16
    a = hip_ctx.featurize_host(_abi.batch_from_rois([r]), CH, s)
    z = dict(r, inten=r["inten"].copy())
    z["inten"][0] = 0
    assert same(hip_ctx.featurize_host(_abi.batch_from_rois([z, r]), CH, s)[1:], a)
    assert same(hip_ctx.featurize_host(_abi.batch_from_rois([z]), CH, s), chords_ref.table(_abi.batch_from_rois([z])))


def test_tile_path_and_device_budget(hip_ctx):
    it, lab = radial_cases.tile()
    b = chords_cases.batch("tile")
    s = _abi.default_settings(64)
    alone = hip_ctx.featurize_host(b, CH, s)
    labels, T = hip_ctx.featurize_tile_host(it, lab, CH, s)
    assert list(labels) == list(b.roi_label) and same(T, alone)
    assert same(T, GOLD["tile"]["table"])
    mask = CH | CAL | OUTLINE | _abi.FAM_INTENSITY | _abi.FAM_GLCM | _abi.FAM_SMOMS
    names = _lib.column_names(mask, s)
    I, M = np.stack([it] * 5), np.stack([lab] * 5)
    one = hip_ctx.featurize_tiles_host(I, M, mask, s, max_device_bytes=1 << 34)
    many = hip_ctx.featurize_tiles_host(I, M, mask, s, max_device_bytes=2 << 20)
    assert (one[0] == many[0]).all() and (one[1] == many[1]).all() and same(one[2], many[2])
    idx = [i for i, n in enumerate(names) if n in chords_ref.NAMES]
    assert same(many[2][:, idx], np.tile(alone, (5, 1)))
    plain = hip_ctx.featurize_tiles_host(I, M, mask & ~CH, s, max_device_bytes=2 << 20)
    rest = [i for i in range(len(names)) if i not in set(idx)]
    assert same(plain[2], many[2][:, rest])


def test_through_nyxus_featurize():
    api = json.load(open(os.path.join(ROOT, "tests", "golden", "chords", "api_expected.json")))
    it, lab = radial_cases.tile()
    for case in api["cases"].values():
        nyx = nyxus_amd.Nyxus(case["features"])
        df = nyx.featurize(it.astype(api["inten_dtype"]), lab)
        assert list(df.columns[-len(case["columns"]):]) == case["columns"]
        assert list(df["ROI_label"]) == api["labels"]
        got = df[case["columns"]].values.astype(float)
        want = np.array(case["numeric"])
        full_g, full_w = np.zeros((len(got), 16)), np.zeros((len(got), 16))
        for j, c in enumerate(case["columns"]):
            full_g[:, chords_ref.NAMES.index(c)], full_w[:, chords_ref.NAMES.index(c)] = got[:, j], want[:, j]
        bad = mismatches(full_g, full_w)
        assert not bad, "\n".join(bad[:10])
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["PERIMETER"])


def test_unassigned_bits_are_still_bad_masks(hip_ctx):
    b = chords_cases.batch("degenerate")
    for bit in (12, 14, 31):
        with pytest.raises(_lib.NyxHipError) as ei:
            hip_ctx.featurize_host(b, CH | (1 << bit), _abi.default_settings(8))
        assert ei.value.code == 1
