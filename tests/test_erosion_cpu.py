"""MAJOR_AXIS_LENGTH .. ROUNDNESS (NYXHIP_FAM_ELLIPSE) and EROSIONS_2_VANISH[_COMPLEMENT] (NYXHIP_FAM_EROSION), the parts that need no
GPU: the column catalogue, the feature-set plumbing, and tests/erosion_ref.py against values recorded from the reference's own
EllipseFittingFeature and ErosionPixelsFeature (tests/golden/erosion)."""
import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset
from tests import erosion_cases, erosion_ref, parity

EL, ER = _abi.FAM_ELLIPSE, _abi.FAM_EROSION
BOTH = EL | ER
CAL = _abi.FAM_FERET | _abi.FAM_MARTIN | _abi.FAM_NASSENSTEIN
OUTLINE = _abi.FAM_FRACTAL | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS
EVERYTHING = _abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE | CAL | _abi.FAM_CHORDS
GOLD = erosion_cases.golden()
ECC, ORI = erosion_ref.NAMES.index("ECCENTRICITY"), erosion_ref.NAMES.index("ORIENTATION")


def mismatches(got, want, compared, rel=parity.REL_TOL):
    """Rows / columns of two (n, 8) tables beyond the bounds of these tests: the erosion columns exactly (as doubles), the ellipse
    columns within `rel` where `compared`; every value finite, 0 <= ECCENTRICITY <= 1, |ORIENTATION| <= 90, compared or not."""
    bad = []
    for c, name in enumerate(erosion_ref.NAMES):
        g, w = got[:, c], want[:, c]
        ok = (g == w) if name in erosion_ref.EROSION else ((np.abs(g - w) <= rel * np.abs(w)) | ~compared[:, c])
        ok &= np.isfinite(g)
        if c == ECC:
            ok &= (g >= 0) & (g <= 1)
        if c == ORI:
            ok &= np.abs(g) <= 90
        bad += [f"row {r} {name}: got {g[r]!r}, want {w[r]!r}" for r in np.nonzero(~ok)[0]]
    return bad


def test_bits_and_column_counts():
    assert EL == 1 << 22 and ER == 1 << 23
    assert _abi.FAM_ALL == 0xFFF and _abi.FAM_NORTH_STAR == 0x7F and not (_abi.FAM_ALL & BOTH) and not (_abi.FAM_NEEDS_ORIGIN & BOTH)
    lib = _lib.load()
    assert lib.nyxhip_abi_version() == 2
    s = _abi.default_settings(64)
    for m in (_abi.FAM_ALL, CAL, _abi.FAM_EULER, EVERYTHING):
        assert lib.nyxhip_n_columns(m | EL, s) == lib.nyxhip_n_columns(m, s) + 6
        assert lib.nyxhip_n_columns(m | ER, s) == lib.nyxhip_n_columns(m, s) + 2
        assert lib.nyxhip_n_columns(m | BOTH, s) == lib.nyxhip_n_columns(m, s) + 8
    assert _lib.column_names(EL, s) == erosion_ref.ELLIPSE and _lib.column_names(ER, s) == erosion_ref.EROSION
    assert _lib.column_names(BOTH, s) == erosion_ref.NAMES and len(erosion_ref.NAMES) == 8


def test_columns_sit_between_the_intensity_block_and_the_fractal_dimensions():
    s = _abi.default_settings(64)
    names = _lib.column_names(EVERYTHING | BOTH, s)
    i = names.index
    assert i("UNIFORMITY_PIU") + 1 == i("MAJOR_AXIS_LENGTH") and i("EROSIONS_2_VANISH_COMPLEMENT") + 1 == i("FRACT_DIM_BOXCOUNT")
    assert names[i("MAJOR_AXIS_LENGTH"):i("FRACT_DIM_BOXCOUNT")] == erosion_ref.NAMES
    # every mask without the bits keeps its columns; with them the other columns keep their order
    for m in (_abi.FAM_ALL, EVERYTHING, _abi.FAM_INTENSITY | _abi.FAM_GLCM, OUTLINE, CAL, _abi.FAM_EULER, _abi.FAM_CHORDS, _abi.FAM_RADIAL | _abi.FAM_GABOR):
        for bits in (EL, ER, BOTH):
            assert [n for n in _lib.column_names(m | bits, s) if n not in erosion_ref.NAMES] == _lib.column_names(m, s)
    assert _lib.column_names(ER | _abi.FAM_GLCM | _abi.FAM_FRACTAL, s)[:5] == erosion_ref.EROSION + ["FRACT_DIM_BOXCOUNT", "FRACT_DIM_PERIMETER", "GLCM_ASM_0"]


def test_unassigned_bits_stay_out_of_the_catalogue():
    s = _abi.default_settings(64)
    for bit in (12, 14, 31):
        assert _lib.column_names(1 << bit, s) == []
        assert _lib.column_names(BOTH | (1 << bit), s) == erosion_ref.NAMES


def test_expand_order_and_the_frozen_lists():
    assert featureset.ELLIPSE == erosion_ref.ELLIPSE and featureset.EROSION == erosion_ref.EROSION
    assert all(featureset.FAMILY_OF[n] == EL for n in erosion_ref.ELLIPSE) and all(featureset.FAMILY_OF[n] == ER for n in erosion_ref.EROSION)
    new = set(erosion_ref.NAMES)
    for frozen in (featureset.ENUM_ORDER, featureset.OUTPUT_ORDER, featureset.SERVED_ORDER, featureset.CATALOGUE_ORDER):
        assert not new & set(frozen)                                         # the earlier lists keep the codes they had
    assert [n for n in featureset.FULL_ORDER if n not in new] == featureset.CATALOGUE_ORDER
    k = featureset.FULL_ORDER.index("UNIFORMITY_PIU")
    assert featureset.FULL_ORDER[k + 1:k + 9] == erosion_ref.NAMES and featureset.FULL_ORDER[k + 9] == "FRACT_DIM_BOXCOUNT"
    assert not any(new & set(g) for g in featureset.GROUPS.values())         # no group token
    mask, order = featureset.expand(["EULER_NUMBER", "EROSIONS_2_VANISH", "MEAN", "GLCM_ASM", "ORIENTATION", "FRACT_DIM_BOXCOUNT", "MAXCHORDS_MAX"])
    assert mask == _abi.FAM_EULER | ER | _abi.FAM_INTENSITY | _abi.FAM_GLCM | EL | _abi.FAM_FRACTAL | _abi.FAM_CHORDS
    assert order == ["MEAN", "ORIENTATION", "EROSIONS_2_VANISH", "FRACT_DIM_BOXCOUNT", "MAXCHORDS_MAX", "EULER_NUMBER", "GLCM_ASM"]
    s = _abi.default_settings(64)
    names = _lib.column_names(mask, s)
    sel = featureset.column_selector(order, names, [0, 45, 90, 135])
    assert [names[j] for j in sel][:6] == order[:6]
    assert featureset.expand(["roundness"]) == (EL, ["ROUNDNESS"])
    for unserved in ("PERIMETER", "CIRCULARITY", "EDGE_MEAN_INTENSITY", "CONVEX_HULL_AREA", "AREA_PIXELS_COUNT", "EXTREMA_P1_X"):
        with pytest.raises(ValueError, match="not served by the MI355X path") as ei:
            featureset.expand([unserved])
        assert "FRAC_AT_D" in str(ei.value) and "MAXCHORDS" in str(ei.value) and "EROSIONS_2_VANISH" in str(ei.value) and "ECCENTRICITY" in str(ei.value)


def test_nyxus_constructs_with_the_new_codes():
    assert nyxus_amd.Nyxus(["EROSIONS_2_VANISH", "MAJOR_AXIS_LENGTH"]) is not None
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["PERIMETER"])


@pytest.mark.parametrize("name", list(erosion_cases.CASES))
def test_restatement_matches_the_reference_classes(name):
    b = erosion_cases.batch(name)
    g = GOLD[name]
    T = erosion_ref.table(b)
    assert T.shape == g["table"].shape == g["compared"].shape
    assert (T[:, 6:] == g["table"][:, 6:]).all(), np.argwhere(T[:, 6:] != g["table"][:, 6:])[:5]     # the erosion columns bit for bit
    assert (g["table"][:, 7] == 0).all()                                     # the class never assigns the complement
    bad = mismatches(T, g["table"], g["compared"])
    assert not bad, "\n".join(bad[:10])
    assert not mismatches(g["table"], g["table"], g["compared"])             # the reference's own values lie inside the columns' ranges


@pytest.mark.parametrize("name", list(erosion_cases.CASES))
def test_the_compared_mask_is_the_stated_rule_and_stays_under_its_cap(name):
    b = erosion_cases.batch(name)
    g = GOLD[name]
    M = np.array([erosion_ref.compared(x, y, g["table"][r, ORI]) for r, x, y in erosion_ref.rois_of(b)])
    assert (M == g["compared"]).all()
    assert M[:, [0, 1, 2, 5, 6, 7]].all()                                    # only ORIENTATION and ECCENTRICITY can be masked
    masked = ~M.all(1)
    assert not [r for r in erosion_cases.ASYMMETRIC[name] if masked[r]]
    rnd = erosion_cases.random_indices(name, b.n_roi)
    if rnd:
        assert 10 * int(masked[rnd].sum()) <= len(rnd)


def test_named_values_and_thresholds():
    E = {n: GOLD[n]["table"][:, 6] for n in erosion_cases.CASES}
    # 3 x 3, 3 x 9, 9 x 3: empty loops.  4 x 4 has one updated cell, (2, 2), and its neighbours never change: a fixed point, like 5 x 5 and 40 x 7
    assert list(E["boxes"]) == [0, 0, 0, 1000, 1000, 1000]
    assert E["shapes"][6] == 0 and E["shapes"][5] == GOLD["shapes"]["table"][5, 6] > 0      # constant: skipped; zero intensities: mask
    assert (GOLD["shapes_softnan"]["table"] == GOLD["shapes"]["table"]).all()               # every value is finite: soft_nan never shows
    # the bars: the middle column outlives pass 0 only with the carries between words (and, in the narrow boxes, the bar leans on the
    # last column and lives a pass longer)
    assert list(E["shapes"][7:]) == [2, 2, 2, 1, 1]
    assert (E["thin"] == 0).all()
    T = GOLD["thin"]["table"]
    assert T[0, 0] == T[0, 1] and T[0, 2] == 1 and T[0, 4] == 0              # one pixel: a circle
    assert T[1, 4] == 0 and T[2, 4] == 90                                    # a row lies, a column stands
    b = erosion_cases.batch("sizes")
    n = np.diff(b.px_offset.astype(np.int64))
    assert erosion_cases.WAVE_PX == 2048 and n[0] <= 2048 < n[1] < n[2]      # on both sides of the ellipse kernels' switch
    b = erosion_cases.batch("mixed")
    words = [2 * erosion_cases.plane_words(w, h) for w, h in zip(b.bbox_w, b.bbox_h)]
    assert erosion_cases.LDS_WORDS == 8192 and sum(v > 8192 for v in words) == 1 and words[5] > 8192
    assert list(erosion_cases.batch("shapes").bbox_w[7:]) == list(erosion_cases.WIDTHS) == list(erosion_cases.batch("words").bbox_w)
