"""MAXCHORDS_* / ALLCHORDS_* (NYXHIP_FAM_CHORDS), the parts that need no GPU: the column catalogue, the feature-set plumbing, and
tests/chords_ref.py against values recorded from the reference's own ChordsFeature (tests/golden/chords)."""
import math

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset
from tests import caliper_ref, chords_cases, chords_ref, parity

CH = _abi.FAM_CHORDS
CAL = _abi.FAM_FERET | _abi.FAM_MARTIN | _abi.FAM_NASSENSTEIN
OUTLINE = _abi.FAM_FRACTAL | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS
GOLD = chords_cases.golden()


def mismatches(got, want, rel=parity.REL_TOL):
    """Rows / columns of two (n, 16) tables beyond the bounds of the chords tests: MAX, MIN, MEDIAN, MODE and the four angles
    exactly (as doubles), MEAN and STDDEV within `rel`."""
    bad = []
    for c, name in enumerate(chords_ref.NAMES):
        g, w = got[:, c], want[:, c]
        ok = (np.abs(g - w) <= rel * np.abs(w)) if name in chords_ref.APPROX else (g == w)
        bad += [f"row {r} {name}: got {g[r]!r}, want {w[r]!r}" for r in np.nonzero(~ok)[0]]
    return bad


def test_bit_and_column_count():
    assert CH == 1 << 21
    assert _abi.FAM_ALL == 0xFFF and _abi.FAM_NORTH_STAR == 0x7F and not (_abi.FAM_ALL & CH)
    lib = _lib.load()
    assert lib.nyxhip_abi_version() == 2
    s = _abi.default_settings(64)
    for m in (_abi.FAM_ALL, CAL, _abi.FAM_EULER, _abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE | CAL):
        assert lib.nyxhip_n_columns(m | CH, s) == lib.nyxhip_n_columns(m, s) + 16
    assert _lib.column_names(CH, s) == chords_ref.NAMES and len(chords_ref.NAMES) == 16


def test_columns_sit_between_the_nassenstein_columns_and_euler_number():
    s = _abi.default_settings(64)
    names = _lib.column_names(_abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE | CAL | CH, s)
    i = names.index
    assert i("STAT_NASSENSTEIN_DIAM_MODE") + 1 == i("MAXCHORDS_MAX") and i("ALLCHORDS_STDDEV") + 1 == i("EULER_NUMBER")
    assert names[i("MAXCHORDS_MAX"):i("EULER_NUMBER")] == chords_ref.NAMES
    # every mask without the bit keeps its columns; with it the other columns keep their order
    for m in (_abi.FAM_ALL, _abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE | CAL, _abi.FAM_INTENSITY | _abi.FAM_GLCM, OUTLINE, CAL, _abi.FAM_EULER):
        assert [n for n in _lib.column_names(m | CH, s) if n not in chords_ref.NAMES] == _lib.column_names(m, s)
    assert _lib.column_names(CH | _abi.FAM_GLCM | _abi.FAM_FRACTAL, s)[:19] == ["FRACT_DIM_BOXCOUNT", "FRACT_DIM_PERIMETER"] + chords_ref.NAMES + ["GLCM_ASM_0"]


def test_unassigned_bits_stay_out_of_the_catalogue():
    s = _abi.default_settings(64)
    for bit in (12, 14, 31):
        assert _lib.column_names(1 << bit, s) == []
        assert _lib.column_names(CH | (1 << bit), s) == chords_ref.NAMES


def test_expand_order_and_the_frozen_lists():
    assert featureset.CHORDS == chords_ref.NAMES
    assert all(featureset.FAMILY_OF[n] == CH for n in chords_ref.NAMES)
    assert not set(chords_ref.NAMES) & set(featureset.SERVED_ORDER)          # the earlier lists keep the codes they had
    assert [n for n in featureset.CATALOGUE_ORDER if n not in chords_ref.NAMES] == featureset.SERVED_ORDER
    k = featureset.CATALOGUE_ORDER.index("STAT_NASSENSTEIN_DIAM_MODE")
    assert featureset.CATALOGUE_ORDER[k + 1:k + 17] == chords_ref.NAMES and featureset.CATALOGUE_ORDER[k + 17] == "EULER_NUMBER"
    assert not any(set(chords_ref.NAMES) & set(g) for g in featureset.GROUPS.values())      # no group token
    mask, order = featureset.expand(["EULER_NUMBER", "ALLCHORDS_MODE", "MEAN", "GLCM_ASM", "MAXCHORDS_MAX_ANG", "STAT_MARTIN_DIAM_MODE"])
    assert mask == _abi.FAM_EULER | CH | _abi.FAM_INTENSITY | _abi.FAM_GLCM | _abi.FAM_MARTIN
    assert order == ["MEAN", "STAT_MARTIN_DIAM_MODE", "MAXCHORDS_MAX_ANG", "ALLCHORDS_MODE", "EULER_NUMBER", "GLCM_ASM"]
    s = _abi.default_settings(64)
    names = _lib.column_names(mask, s)
    sel = featureset.column_selector(order, names, [0, 45, 90, 135])
    assert [names[j] for j in sel][:5] == order[:5]
    assert featureset.expand(["allchords_median"]) == (CH, ["ALLCHORDS_MEDIAN"])
    for unserved in ("PERIMETER", "CIRCULARITY", "EDGE_MEAN_INTENSITY", "CONVEX_HULL_AREA", "AREA_PIXELS_COUNT", "EXTREMA_P1_X"):
        with pytest.raises(ValueError, match="not served by the MI355X path") as ei:
            featureset.expand([unserved])
        assert "FRAC_AT_D" in str(ei.value) and "MAXCHORDS" in str(ei.value)


def test_nyxus_constructs_with_a_chords_code():
    nyx = nyxus_amd.Nyxus(["MAXCHORDS_MAX"])
    assert nyx is not None
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["PERIMETER"])


def test_the_angle_table_is_the_loop_of_the_reference():
    a = chords_ref.angles()
    assert len(a) == 20 and a[0] == 0.0 and a[-1] < math.pi
    assert a[-1] + math.pi / 20.0 == math.pi                                # the 20th sum is M_PI itself: the loop ends there
    assert any(a[k] != k * math.pi / 20.0 for k in range(20))               # ... and the partial sums are not k * pi / 20


@pytest.mark.parametrize("name", list(chords_cases.CASES))
def test_restatement_matches_the_reference_class(name):
    b = chords_cases.batch(name)
    g = GOLD[name]
    P = chords_ref.batch_per_angle(b)
    assert len(P) == len(g["table"]) == b.n_roi
    for r in range(b.n_roi):
        mx, cnt, sm = chords_ref.summary(P[r])
        assert (mx == g["max"][r]).all() and (cnt == g["count"][r]).all() and (sm == g["sum"][r]).all(), r
    ang = chords_ref.angles()
    T = np.array([chords_ref.close(p, ang) for p in P]).reshape(b.n_roi, 16)
    assert (T == g["table"]).all(), np.argwhere(T != g["table"])[:5]        # every column, MEAN and STDDEV included, bit for bit


def test_degenerate_rows_and_soft_nan():
    T = GOLD["degenerate"]["table"]
    assert (GOLD["degenerate_softnan"]["table"] == T).all()                  # every value is finite: soft_nan never shows
    assert (T[0] == 0).all() and (T[1] == 0).all()                           # 1 pixel, 1 x 2: no closed chord at any angle
    assert (GOLD["degenerate"]["count"][0] == 0).all()
    # a 1 x 5 row at angle 0 is five columns of one cell each, all touching the last row: no chord there
    assert GOLD["degenerate"]["count"][2][0] == 0 and GOLD["degenerate"]["count"][2].sum() > 0
    Z = GOLD["zeros"]
    assert (Z["table"][1] == 0).all() and (Z["count"][1] == 0).all()         # nothing but zero intensities
    assert (Z["table"][2] != Z["table"][3]).any()                           # the cloud order decides cells shared with a zero pixel


def test_the_placement_changes_the_reference_values():
    P = GOLD["placed"]["table"].reshape(3, 8, 16)
    assert (P[0] != P[1]).any() and (P[0] != P[2]).any()
    b = chords_cases.batch("placed")
    z = np.zeros(b.n_roi, np.int64)
    assert (chords_ref.table(b, origin=(z, z))[8:16] == P[0]).all()          # without origins: the rows of the first placement


def test_step_and_limit_cases_straddle_their_thresholds():
    b = chords_cases.batch("step")
    assert list(b.bbox_w[:3]) == [199, 200, 201] and b.bbox_w[3] == 221
    scanned = []
    for r in range(3):                                                       # angle 0: every column, then every second one
        x, y, v = b.x[b.px_offset[r]:b.px_offset[r + 1]], b.y[b.px_offset[r]:b.px_offset[r + 1]], b.inten[b.px_offset[r]:b.px_offset[r + 1]]
        xi, yi = chords_ref.rotated_cells(x, y, b.origin_x[r], b.origin_y[r], b.bbox_w[r], b.bbox_h[r], 0.0, 1.0)
        scanned.append(len(chords_ref.column_chords(xi, yi, v)[0]))
    assert scanned == [199, 100, 101]
    # (a column of the band has a chord at angle 0 only where its bottom cell is missing: a run on the last row is dropped
    # -- columns 1, 5, 9, ...: 50 of the 199; with step 2 only even columns are scanned, and none of them has one)
    assert list(GOLD["step"]["count"][:3, 0]) == [50, 0, 0]
    assert chords_cases.LDS_WORDS == 8192
    b = chords_cases.batch("limit")
    words = [chords_cases.plane_words(w, h) for w, h in zip(b.bbox_w, b.bbox_h)]
    assert all(v <= 8192 for v in words[:6]) and all(v > 8192 for v in words[6:])
    assert max(words[:6]) == 8192 and min(words[6:]) == 513 * 17            # just below, just above
