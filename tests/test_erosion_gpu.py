"""The ellipse and erosion columns on the GPU: the HIP rows against values recorded from the reference's own classes
(tests/golden/erosion), against tests/erosion_ref.py, and against themselves across every way a row can be requested.  The erosion
columns are compared exactly; the ellipse columns at parity.REL_TOL under the recorded `compared` mask (integer sums: a row has the
same bits whichever kernel, call or batch served it)."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import erosion_cases, erosion_ref
from tests.test_erosion_cpu import mismatches

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EL, ER = _abi.FAM_ELLIPSE, _abi.FAM_EROSION
BOTH = EL | ER
CAL = _abi.FAM_FERET | _abi.FAM_MARTIN | _abi.FAM_NASSENSTEIN
OUTLINE = _abi.FAM_FRACTAL | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS
GOLD = erosion_cases.golden()
_ROWS = {}


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def rows(ctx, name):
    """The eight columns of a case, computed once and shared."""
    if name not in _ROWS:
        _ROWS[name] = ctx.featurize_host(erosion_cases.batch(name), BOTH, _abi.default_settings(64))
    return _ROWS[name]


def split(ctx, b, mask, s):
    """(the new columns, the other columns, their names) of one call."""
    names = _lib.column_names(mask, s)
    T = ctx.featurize_host(b, mask, s)
    idx = [i for i, n in enumerate(names) if n in erosion_ref.NAMES]
    rest = [i for i in range(len(names)) if i not in set(idx)]
    return T[:, idx], T[:, rest], [names[i] for i in rest]


@pytest.mark.parametrize("name", list(erosion_cases.CASES))
def test_hip_rows_match_the_reference_classes(hip_ctx, name):
    want, cmp_ = GOLD[name]["table"], GOLD[name]["compared"]
    got = rows(hip_ctx, name)
    assert got.shape == want.shape
    rel = np.where(cmp_[:, :6], np.abs(got[:, :6] - want[:, :6]) / np.maximum(np.abs(want[:, :6]), 1e-300), 0)
    print(f"{name}: {len(got)} ROIs; erosion values {sorted(set(got[:, 6]))}; largest relative difference per ellipse column {rel.max(0)}")
    bad = mismatches(got, want, cmp_)
    assert not bad, "\n".join(bad[:10])
    assert (got[:, 6] == want[:, 6]).all() and (got[:, 7] == 0.0).all()


def test_rows_are_repeatable_and_independent_of_the_batch(hip_ctx):
    s = _abi.default_settings(64)
    for name in ("shapes", "thin", "sizes", "mixed"):
        rois = erosion_cases.CASES[name]()
        first = rows(hip_ctx, name)
        assert same(hip_ctx.featurize_host(_abi.batch_from_rois(rois), BOTH, s), first), name
        for r in range(len(rois)):
            if name == "mixed" and r != 5:
                continue                                                     # the large ROI alone: only the list launch has work
            assert same(hip_ctx.featurize_host(_abi.batch_from_rois(rois[r:r + 1]), BOTH, s), first[r:r + 1]), (name, r)
    # the large ROI: alone (case "large") and beside small ones (case "mixed")
    assert same(rows(hip_ctx, "large"), rows(hip_ctx, "mixed")[5:6])
    # the restatement's ellipse operations are the device's: every column but ORIENTATION (atan) bit for bit
    for name in ("thin", "sizes", "words"):
        R = erosion_ref.table(erosion_cases.batch(name))
        assert same(rows(hip_ctx, name)[:, [0, 1, 2, 3, 5, 6, 7]], R[:, [0, 1, 2, 3, 5, 6, 7]]), name


def test_each_bit_alone_and_both_together(hip_ctx):
    s = _abi.default_settings(64)
    for name in ("boxes", "shapes", "mixed"):
        b = erosion_cases.batch(name)
        both = rows(hip_ctx, name)
        assert same(hip_ctx.featurize_host(b, EL, s), both[:, :6]) and same(hip_ctx.featurize_host(b, ER, s), both[:, 6:]), name


def test_neighbours_keep_their_columns(hip_ctx):
    """The moved column bases and the zeroed span: beside other families every old column is the one of the call without the two
    bits, bit for bit, and the new columns are the ones of the call alone."""
    b = _abi.batch_from_rois(erosion_cases.shapes() + erosion_cases.thin() + erosion_cases.sizes()[:2] + erosion_cases.words()[:2])
    s = _abi.default_settings(64)
    alone = hip_ctx.featurize_host(b, BOTH, s)
    extras = [_abi.FAM_INTENSITY | _abi.FAM_GLCM | _abi.FAM_FRACTAL | _abi.FAM_CHORDS,
              _abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE | CAL | _abi.FAM_CHORDS,
              _abi.FAM_GLCM, CAL | _abi.FAM_EULER, _abi.FAM_RADIAL | _abi.FAM_GABOR | _abi.FAM_SMOMS]
    for extra in extras:
        plain = hip_ctx.featurize_host(b, extra, s)
        for bits, cols in ((BOTH, slice(0, 8)), (EL, slice(0, 6)), (ER, slice(6, 8))):
            got, rest, rest_names = split(hip_ctx, b, extra | bits, s)
            assert rest_names == _lib.column_names(extra, s)
            assert same(got, alone[:, cols]), (extra, bits, np.argwhere(got != alone[:, cols])[:5])
            assert same(plain, rest), (extra, bits, np.argwhere(~((plain == rest) | (np.isnan(plain) & np.isnan(rest))))[:5])


def test_soft_nan_never_shows(hip_ctx):
    s = _abi.default_settings(64)
    s.soft_nan = -7.5
    for name in ("shapes", "thin", "boxes"):
        got = hip_ctx.featurize_host(erosion_cases.batch(name), BOTH, s)
        assert same(got, rows(hip_ctx, name)) and np.isfinite(got).all()
    assert not mismatches(rows(hip_ctx, "shapes"), GOLD["shapes_softnan"]["table"], GOLD["shapes"]["compared"])


def test_tile_path(hip_ctx):
    it, lab = erosion_cases.tile()
    b = erosion_cases.batch("tile")
    s = _abi.default_settings(64)
    for bits, cols in ((BOTH, slice(0, 8)), (ER, slice(6, 8)), (EL, slice(0, 6))):
        labels, T = hip_ctx.featurize_tile_host(it, lab, bits, s)
        assert list(labels) == list(b.roi_label) and same(T, rows(hip_ctx, "tile")[:, cols])
    mask = BOTH | _abi.FAM_INTENSITY | _abi.FAM_GLCM | _abi.FAM_FRACTAL
    names = _lib.column_names(mask, s)
    I, M = np.stack([it] * 3), np.stack([lab] * 3)
    many = hip_ctx.featurize_tiles_host(I, M, mask, s, max_device_bytes=2 << 20)
    idx = [i for i, n in enumerate(names) if n in erosion_ref.NAMES]
    rest = [i for i in range(len(names)) if i not in set(idx)]
    assert same(many[2][:, idx], np.tile(rows(hip_ctx, "tile"), (3, 1)))
    plain = hip_ctx.featurize_tiles_host(I, M, mask & ~BOTH, s, max_device_bytes=2 << 20)
    assert same(plain[2], many[2][:, rest])


def test_through_nyxus_featurize():
    api = json.load(open(os.path.join(ROOT, "tests", "golden", "erosion", "api_expected.json")))
    it, lab = erosion_cases.tile()
    for case in api["cases"].values():
        nyx = nyxus_amd.Nyxus(case["features"])
        df = nyx.featurize(it.astype(api["inten_dtype"]), lab)
        assert list(df.columns[-len(case["columns"]):]) == case["columns"]
        assert list(df["ROI_label"]) == api["labels"]
        got = df[case["columns"]].values.astype(float)
        want, cmp_ = np.array(case["numeric"]), np.array(case["compared"], bool)
        full_g, full_w, full_c = np.zeros((len(got), 8)), np.zeros((len(got), 8)), np.ones((len(got), 8), bool)
        for j, c in enumerate(case["columns"]):
            k = erosion_ref.NAMES.index(c)
            full_g[:, k], full_w[:, k], full_c[:, k] = got[:, j], want[:, j], cmp_[:, j]
        bad = mismatches(full_g, full_w, full_c)
        assert not bad, "\n".join(bad[:10])
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["PERIMETER"])


def test_unassigned_bits_are_still_bad_masks(hip_ctx):
    b = erosion_cases.batch("thin")
    for bit in (12, 14, 31):
        for bits in (EL, ER, BOTH):
            with pytest.raises(_lib.NyxHipError) as ei:
                hip_ctx.featurize_host(b, bits | (1 << bit), _abi.default_settings(8))
            assert ei.value.code == 1
