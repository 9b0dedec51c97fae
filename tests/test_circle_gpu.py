"""The circle and geodetic columns on the GPU: the HIP rows against values recorded from the reference's own classes
(tests/golden/circle) at parity.REL_TOL, against tests/circle_ref.py bit for bit, and against themselves across every way a row can
be requested (a row has the same bits whichever launch, call or batch served it: every decision is the reference's float or integer
comparison, every sum has the reference's order)."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import circle_cases, circle_ref, parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CI, GE = _abi.FAM_CIRCLES, _abi.FAM_GEODETIC
BOTH = CI | GE
CAL = _abi.FAM_FERET | _abi.FAM_MARTIN | _abi.FAM_NASSENSTEIN
OUTLINE = _abi.FAM_FRACTAL | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS
GOLD = circle_cases.golden()
_ROWS = {}


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def rows(ctx, name):
    """The five columns of a case, computed once and shared."""
    if name not in _ROWS:
        _ROWS[name] = ctx.featurize_host(circle_cases.batch(name), BOTH, _abi.default_settings(64))
    return _ROWS[name]


def split(ctx, b, mask, s):
    """(the new columns, the other columns, their names) of one call."""
    names = _lib.column_names(mask, s)
    T = ctx.featurize_host(b, mask, s)
    idx = [i for i, n in enumerate(names) if n in circle_ref.NAMES]
    rest = [i for i in range(len(names)) if i not in set(idx)]
    return T[:, idx], T[:, rest], [names[i] for i in rest]


@pytest.mark.parametrize("name", list(circle_cases.CASES))
def test_hip_rows_match_the_reference_classes(hip_ctx, name):
    want = GOLD[name]["table"][:, :5]
    got = rows(hip_ctx, name)
    assert got.shape == want.shape and np.isfinite(got).all()
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print(f"{name}: {len(got)} ROIs; largest relative difference per column {rel.max(0)}; values that differ in a bit: {int((got != want).sum())}")
    assert (np.abs(got - want) <= parity.REL_TOL * np.abs(want)).all(), np.argwhere(np.abs(got - want) > parity.REL_TOL * np.abs(want))[:8]


@pytest.mark.parametrize("name", list(circle_cases.CASES))
def test_hip_rows_match_the_restatement_bit_for_bit(hip_ctx, name):
    R = circle_ref.table(circle_cases.batch(name))[:, :5]
    got = rows(hip_ctx, name)
    assert same(got, R), [(r, circle_ref.NAMES[c], got[r, c], R[r, c]) for r, c in np.argwhere(got != R)[:8]]


def test_rows_are_repeatable_and_independent_of_the_batch(hip_ctx):
    s = _abi.default_settings(64)
    for name in ("small", "shapes", "words"):
        rois = circle_cases.CASES[name]()
        first = rows(hip_ctx, name)
        assert same(hip_ctx.featurize_host(_abi.batch_from_rois(rois), BOTH, s), first), name
        for r in range(len(rois)):                                           # each ROI alone
            assert same(hip_ctx.featurize_host(_abi.batch_from_rois(rois[r:r + 1]), BOTH, s), first[r:r + 1]), (name, r)
    mixed = rows(hip_ctx, "mixed")
    assert same(hip_ctx.featurize_host(circle_cases.batch("mixed"), BOTH, s), mixed)
    # the long-contour comb (read from the workspace) and the ring (the big-box list chain): alone and beside small ROIs
    assert same(rows(hip_ctx, "long_comb"), mixed[circle_cases.MIXED_COMB:circle_cases.MIXED_COMB + 1])
    assert same(rows(hip_ctx, "ring"), mixed[circle_cases.MIXED_RING:circle_cases.MIXED_RING + 1])


def test_each_bit_alone_and_both_together(hip_ctx):
    s = _abi.default_settings(64)
    for name in ("small", "shapes", "mixed"):
        b = circle_cases.batch(name)
        both = rows(hip_ctx, name)
        assert same(hip_ctx.featurize_host(b, CI, s), both[:, :3]) and same(hip_ctx.featurize_host(b, GE, s), both[:, 3:]), name


def test_placed_through_the_origin_entry_and_without_it(hip_ctx):
    b = circle_cases.batch("placed")
    s = _abi.default_settings(64)
    got = rows(hip_ctx, "placed")
    k = circle_cases.N_PLACED
    assert len(got) == 4 * k and (got[:k, :3] != got[3 * k:, :3]).any()      # the origin is read
    for p in range(1, 4):
        assert same(got[p * k:(p + 1) * k, 3:], got[:k, 3:])                 # NYXHIP_FAM_GEODETIC: identical at every origin
    plain = _abi.HostBatch(b.roi_label, b.px_offset, b.x, b.y, b.inten, b.bbox_w, b.bbox_h, b.min_inten, b.max_inten)
    old = hip_ctx.featurize_host(plain, BOTH, s)                             # nyxhip_featurize_batch: every origin (0, 0)
    assert same(old, np.tile(got[:k], (4, 1)))
    assert same(hip_ctx.featurize_host(plain, GE, s), got[:, 3:])


def test_neighbours_keep_their_columns(hip_ctx):
    """The moved column bases: beside other families every old column is the one of the call without the two bits, bit for bit, and
    the new columns are the ones of the call alone."""
    b = _abi.batch_from_rois(circle_cases.small() + circle_cases.shapes()[:12] + circle_cases.words()[:2] + circle_cases.placed()[9:14])
    s = _abi.default_settings(64)
    alone = hip_ctx.featurize_host(b, BOTH, s)
    extras = [_abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE | CAL | _abi.FAM_CHORDS | _abi.FAM_ELLIPSE | _abi.FAM_EROSION,
              _abi.FAM_GLCM, _abi.FAM_EULER | _abi.FAM_ROI_RADIUS]
    for extra in extras:
        plain = hip_ctx.featurize_host(b, extra, s)
        for bits, cols in ((BOTH, slice(0, 5)), (CI, slice(0, 3)), (GE, slice(3, 5))):
            got, rest, rest_names = split(hip_ctx, b, extra | bits, s)
            assert rest_names == _lib.column_names(extra, s)
            assert same(got, alone[:, cols]), (extra, bits, np.argwhere(got != alone[:, cols])[:5])
            assert same(plain, rest), (extra, bits, np.argwhere(~((plain == rest) | (np.isnan(plain) & np.isnan(rest))))[:5])


def test_soft_nan_never_shows(hip_ctx):
    s = _abi.default_settings(64)
    s.soft_nan = -7.5
    for name in ("small", "shapes"):
        got = hip_ctx.featurize_host(circle_cases.batch(name), BOTH, s)
        assert same(got, rows(hip_ctx, name)) and np.isfinite(got).all()
    want = GOLD["shapes_softnan"]["table"][:, :5]                            # recorded under soft_nan = -7.5: the same finite values
    assert (np.abs(rows(hip_ctx, "shapes") - want) <= parity.REL_TOL * np.abs(want)).all()


def test_tile_path(hip_ctx):
    it, lab = circle_cases.tile()
    b = circle_cases.batch("tile")
    s = _abi.default_settings(64)
    for bits, cols in ((BOTH, slice(0, 5)), (GE, slice(3, 5)), (CI, slice(0, 3))):
        labels, T = hip_ctx.featurize_tile_host(it, lab, bits, s)
        assert list(labels) == list(b.roi_label) and same(T, rows(hip_ctx, "tile")[:, cols])
    mask = BOTH | _abi.FAM_INTENSITY | _abi.FAM_GLCM | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS
    names = _lib.column_names(mask, s)
    I, M = np.stack([it] * 3), np.stack([lab] * 3)
    many = hip_ctx.featurize_tiles_host(I, M, mask, s, max_device_bytes=2 << 20)
    idx = [i for i, n in enumerate(names) if n in circle_ref.NAMES]
    rest = [i for i in range(len(names)) if i not in set(idx)]
    assert same(many[2][:, idx], np.tile(rows(hip_ctx, "tile"), (3, 1)))
    plain = hip_ctx.featurize_tiles_host(I, M, mask & ~BOTH, s, max_device_bytes=2 << 20)
    assert same(plain[2], many[2][:, rest])


def test_through_nyxus_featurize():
    api = json.load(open(os.path.join(ROOT, "tests", "golden", "circle", "api_expected.json")))
    it, lab = circle_cases.tile()
    for case in api["cases"].values():
        nyx = nyxus_amd.Nyxus(case["features"])
        df = nyx.featurize(it.astype(api["inten_dtype"]), lab)
        assert list(df.columns[-len(case["columns"]):]) == case["columns"]
        assert list(df["ROI_label"]) == api["labels"]
        got = df[case["columns"]].values.astype(float)
        want = np.array(case["numeric"])
        assert np.isfinite(got).all() and (np.abs(got - want) <= parity.REL_TOL * np.abs(want)).all()
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["PERIMETER"])


def test_unassigned_bits_are_still_bad_masks(hip_ctx):
    b = circle_cases.batch("small")
    for bit in (12, 14, 26, 27, 28, 29, 30, 31):
        for bits in (CI, GE, BOTH):
            with pytest.raises(_lib.NyxHipError) as ei:
                hip_ctx.featurize_host(b, bits | (1 << bit), _abi.default_settings(8))
            assert ei.value.code == 1
