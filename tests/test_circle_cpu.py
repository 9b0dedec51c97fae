"""DIAMETER_MIN_ENCLOSING_CIRCLE, DIAMETER_CIRCUMSCRIBING_CIRCLE, DIAMETER_INSCRIBING_CIRCLE (NYXHIP_FAM_CIRCLES) and GEODETIC_LENGTH,
THICKNESS (NYXHIP_FAM_GEODETIC), the parts that need no GPU: the column catalogue, the feature-set plumbing, and tests/circle_ref.py
against values recorded from the reference's own classes (tests/golden/circle) -- every value of every ROI, bit for bit."""
import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset
from tests import circle_cases, circle_ref

CI, GE = _abi.FAM_CIRCLES, _abi.FAM_GEODETIC
BOTH = CI | GE
CAL = _abi.FAM_FERET | _abi.FAM_MARTIN | _abi.FAM_NASSENSTEIN
OUTLINE = _abi.FAM_FRACTAL | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS
EVERYTHING = _abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE | CAL | _abi.FAM_CHORDS | _abi.FAM_ELLIPSE | _abi.FAM_EROSION
UNASSIGNED = (12, 14, 26, 27, 28, 29, 30, 31)
GOLD = circle_cases.golden()


def test_bits_and_column_counts():
    assert CI == 1 << 24 and GE == 1 << 25
    assert _abi.FAM_ALL == 0xFFF and _abi.FAM_NORTH_STAR == 0x7F and not (_abi.FAM_ALL & BOTH)
    assert (_abi.FAM_NEEDS_ORIGIN & BOTH) == CI                              # the circle class reads the origin, the geodetic class does not
    lib = _lib.load()
    assert lib.nyxhip_abi_version() == 2
    s = _abi.default_settings(64)
    for m in (_abi.FAM_ALL, CAL, _abi.FAM_EULER, _abi.FAM_ROI_RADIUS, EVERYTHING):
        assert lib.nyxhip_n_columns(m | CI, s) == lib.nyxhip_n_columns(m, s) + 3
        assert lib.nyxhip_n_columns(m | GE, s) == lib.nyxhip_n_columns(m, s) + 2
        assert lib.nyxhip_n_columns(m | BOTH, s) == lib.nyxhip_n_columns(m, s) + 5
    assert _lib.column_names(CI, s) == circle_ref.CIRCLES and _lib.column_names(GE, s) == circle_ref.GEODETIC
    assert _lib.column_names(BOTH, s) == circle_ref.NAMES and len(circle_ref.NAMES) == 5


def test_columns_sit_between_the_euler_number_and_the_roi_radius():
    s = _abi.default_settings(64)
    names = _lib.column_names(EVERYTHING | BOTH, s)
    i = names.index
    assert i("EULER_NUMBER") + 1 == i("DIAMETER_MIN_ENCLOSING_CIRCLE") and i("THICKNESS") + 1 == i("ROI_RADIUS_MEAN")
    assert names[i("EULER_NUMBER") + 1:i("ROI_RADIUS_MEAN")] == circle_ref.NAMES
    # without Euler: behind the chords; without chords: behind the caliper columns; without the radius: in front of GLCM
    names = _lib.column_names(_abi.FAM_CHORDS | BOTH | _abi.FAM_ROI_RADIUS | _abi.FAM_GLCM, s)
    assert names[names.index("ALLCHORDS_STDDEV") + 1:names.index("ROI_RADIUS_MEAN")] == circle_ref.NAMES
    names = _lib.column_names(CAL | _abi.FAM_INTENSITY | GE | _abi.FAM_GLCM, s)
    assert names[names.index("STAT_NASSENSTEIN_DIAM_MODE") + 1:names.index("GLCM_ASM_0")] == circle_ref.GEODETIC
    assert _lib.column_names(_abi.FAM_EULER | CI | _abi.FAM_ROI_RADIUS, s) == ["EULER_NUMBER"] + circle_ref.CIRCLES + featureset.ROI_RADIUS
    # every mask without the bits keeps its columns; with them the other columns keep their order
    for m in (_abi.FAM_ALL, EVERYTHING, _abi.FAM_INTENSITY | _abi.FAM_GLCM, OUTLINE, CAL, _abi.FAM_EULER, _abi.FAM_CHORDS, _abi.FAM_ROI_RADIUS,
              _abi.FAM_RADIAL | _abi.FAM_GABOR, _abi.FAM_EULER | _abi.FAM_CHORDS | _abi.FAM_ROI_RADIUS):
        for bits in (CI, GE, BOTH):
            assert [n for n in _lib.column_names(m | bits, s) if n not in circle_ref.NAMES] == _lib.column_names(m, s)


def test_unassigned_bits_stay_out_of_the_catalogue():
    s = _abi.default_settings(64)
    for bit in UNASSIGNED:
        assert _lib.column_names(1 << bit, s) == []
        assert _lib.column_names(BOTH | (1 << bit), s) == circle_ref.NAMES


def test_expand_order_and_the_frozen_lists():
    assert featureset.CIRCLES == circle_ref.CIRCLES and featureset.GEODETIC == circle_ref.GEODETIC
    assert all(featureset.FAMILY_OF[n] == CI for n in circle_ref.CIRCLES) and all(featureset.FAMILY_OF[n] == GE for n in circle_ref.GEODETIC)
    new = set(circle_ref.NAMES)
    for frozen in (featureset.ENUM_ORDER, featureset.OUTPUT_ORDER, featureset.SERVED_ORDER, featureset.CATALOGUE_ORDER, featureset.FULL_ORDER):
        assert not new & set(frozen)                                         # the earlier lists keep the codes they had
    assert [n for n in featureset.EXPAND_ORDER if n not in new] == featureset.FULL_ORDER
    k = featureset.EXPAND_ORDER.index("EULER_NUMBER")
    assert featureset.EXPAND_ORDER[k + 1:k + 6] == circle_ref.NAMES and featureset.EXPAND_ORDER[k + 6] == "ROI_RADIUS_MEAN"
    assert not any(new & set(g) for g in featureset.GROUPS.values())         # no group token
    mask, order = featureset.expand(["ROI_RADIUS_MAX", "THICKNESS", "MEAN", "GLCM_ASM", "DIAMETER_INSCRIBING_CIRCLE", "EULER_NUMBER", "ROUNDNESS"])
    assert mask == _abi.FAM_ROI_RADIUS | GE | _abi.FAM_INTENSITY | _abi.FAM_GLCM | CI | _abi.FAM_EULER | _abi.FAM_ELLIPSE
    assert order == ["MEAN", "ROUNDNESS", "EULER_NUMBER", "DIAMETER_INSCRIBING_CIRCLE", "THICKNESS", "ROI_RADIUS_MAX", "GLCM_ASM"]
    s = _abi.default_settings(64)
    names = _lib.column_names(mask, s)
    sel = featureset.column_selector(order, names, [0, 45, 90, 135])
    assert [names[j] for j in sel][:6] == order[:6]
    assert featureset.expand(["thickness"]) == (GE, ["THICKNESS"])
    for unserved in ("PERIMETER", "CIRCULARITY", "EDGE_MEAN_INTENSITY", "CONVEX_HULL_AREA", "AREA_PIXELS_COUNT", "EXTREMA_P1_X"):
        with pytest.raises(ValueError, match="not served by the MI355X path") as ei:
            featureset.expand([unserved])
        text = str(ei.value)
        assert "FRAC_AT_D" in text and "MAXCHORDS" in text and "EROSIONS_2_VANISH" in text and "ECCENTRICITY" in text
        assert all(n in text for n in circle_ref.NAMES)


def test_nyxus_constructs_with_the_new_codes():
    assert nyxus_amd.Nyxus(["GEODETIC_LENGTH", "DIAMETER_INSCRIBING_CIRCLE"]) is not None
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["PERIMETER"])


@pytest.mark.parametrize("name", list(circle_cases.CASES))
def test_restatement_matches_the_reference_classes(name):
    """All five columns and the recorded perimeter and centroid, every ROI, bit for bit."""
    b = circle_cases.batch(name)
    g = GOLD[name]
    T, flags = circle_ref.table(b, with_flags=True)
    assert T.shape == g["table"].shape == (b.n_roi, 8)
    assert np.isfinite(g["table"]).all()
    assert (T == g["table"]).all(), [(r, (circle_ref.NAMES + circle_ref.EXTRA)[c], T[r, c], g["table"][r, c]) for r, c in np.argwhere(T != g["table"])[:8]]
    assert (flags == g["clamped"]).all()
    from tests.radial_ref import contours_of
    assert [len(k) for k in contours_of(b)] == g["n_contour"].tolist()


def test_named_values_and_branches():
    S = GOLD["small"]
    assert S["n_contour"].tolist() == [0, 0, 3, 2, 3, 0]                     # 1 px, 2 px, 3 in a row, 3 in an L, 2 x 2, an anti-diagonal
    assert (S["table"][[0, 1, 5], :5] == 0).all()                            # no contour: the circle class is skipped, the perimeter is 0
    assert (S["table"][[2, 3, 4], :3] > 0).all()
    assert S["table"][3, 0] == 2.0 * float(np.float32(0.5) + np.float32(1e-4))   # the two-point branch: two points one apart, radius 1 / 2 + EPS
    assert (GOLD["shapes_softnan"]["table"] == GOLD["shapes"]["table"]).all()                # every value is finite: soft_nan never shows
    # both branches of SqRootTmp < 0: compact shapes clamp it, needles and combs do not
    sh = GOLD["shapes"]["clamped"]
    assert not sh[0] and not sh[1] and sh[3] and sh[4]                       # the two needles | the two discs
    assert not GOLD["long_comb"]["clamped"][0]
    clamped = GOLD["shapes"]["table"][sh]
    assert (clamped[:, 3] * 4.0 == clamped[:, 5]).all()                      # clamped: GEODETIC_LENGTH = PERIMETER / 4 (+ sqrt(0))
    # the ballot word boundaries, the contour beyond the LDS bound, the box beyond the LDS contour plane
    assert GOLD["words"]["n_contour"].tolist() == [63, 64, 65, 128, 129] == sorted(circle_cases.WORD_BOXES)
    assert circle_cases.CONTOUR_LDS == 2048 and GOLD["long_comb"]["n_contour"][0] > 2048
    b = circle_cases.batch("mixed")
    big = [(int(w) + 2) * (int(h) + 2) > 16384 for w, h in zip(b.bbox_w, b.bbox_h)]
    assert [i for i, v in enumerate(big) if v] == [circle_cases.MIXED_RING]
    assert GOLD["mixed"]["n_contour"][circle_cases.MIXED_COMB] > 2048
    assert (GOLD["mixed"]["table"][circle_cases.MIXED_RING] == GOLD["ring"]["table"][0]).all()
    assert (GOLD["mixed"]["table"][circle_cases.MIXED_COMB] == GOLD["long_comb"]["table"][0]).all()


def test_placed_values_move_with_the_origin_and_the_geodetic_pair_does_not():
    T = GOLD["placed"]["table"]
    k = circle_cases.N_PLACED
    assert len(T) == 4 * k and len(circle_cases.PLACEMENTS) == 4
    base = T[:k]
    for p in range(4):
        P = T[p * k:(p + 1) * k]
        assert (P[:, 3:6] == base[:, 3:6]).all()                             # GEODETIC_LENGTH, THICKNESS, PERIMETER: differences only
    assert (T[:k, :3] != T[3 * k:, :3]).any()                                # beyond 2^24 the circle columns are other values
