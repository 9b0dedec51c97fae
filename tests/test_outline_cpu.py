"""Fractal dimension, Euler number and ROI radius (NYXHIP_FAM_FRACTAL / _EULER / _ROI_RADIUS), the parts that need no GPU: the
column catalogue, the feature-set plumbing, and tests/outline_ref.py against tables recorded from the reference's own classes
(tests/golden/outline)."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib, featureset
from tests import outline_cases, outline_ref, parity

F, E, RR = _abi.FAM_FRACTAL, _abi.FAM_EULER, _abi.FAM_ROI_RADIUS
NEW = F | E | RR


def test_bits_and_column_counts():
    assert (F, E, RR) == (1 << 15, 1 << 16, 1 << 17)
    assert _abi.FAM_ALL == 0xFFF and _abi.FAM_NORTH_STAR == 0x7F and not (_abi.FAM_ALL & NEW)
    lib = _lib.load()
    assert lib.nyxhip_abi_version() == 2
    s = _abi.default_settings(64)
    assert [len(_lib.column_names(m, s)) for m in (F, E, RR, NEW)] == [2, 1, 3, 6]
    assert _lib.column_names(NEW, s) == outline_cases.NAMES == outline_ref.NAMES


def test_columns_sit_between_the_intensity_block_and_glcm():
    s = _abi.default_settings(64)
    names = _lib.column_names(_abi.FAM_ALL | _abi.FAM_RADIAL | NEW, s)
    i = names.index
    assert i("UNIFORMITY_PIU") + 1 == i("FRACT_DIM_BOXCOUNT") and i("FRACT_DIM_PERIMETER") + 1 == i("EULER_NUMBER")
    assert i("EULER_NUMBER") + 1 == i("ROI_RADIUS_MEAN") and i("ROI_RADIUS_MEDIAN") + 1 == i("GLCM_ASM_0")
    # a mask without the new bits keeps its columns; with them the old columns keep their order
    old = _lib.column_names(_abi.FAM_ALL | _abi.FAM_RADIAL, s)
    assert [n for n in names if n not in outline_cases.NAMES] == old
    assert _lib.column_names(E | _abi.FAM_GLCM, s)[0] == "EULER_NUMBER"


def test_unassigned_bits_stay_out_of_the_catalogue():
    s = _abi.default_settings(64)
    for bit in (12, 14, 31):
        assert _lib.column_names(1 << bit, s) == []
        assert _lib.column_names(NEW | (1 << bit), s) == outline_cases.NAMES


def test_enum_order_is_untouched_and_expand_has_its_own_order():
    assert not set(outline_cases.NAMES) & set(featureset.ENUM_ORDER)
    assert len(featureset.OUTPUT_ORDER) == len(featureset.ENUM_ORDER) + 6
    k = len(featureset.INTENSITY)
    assert featureset.OUTPUT_ORDER[k:k + 6] == outline_cases.NAMES and featureset.OUTPUT_ORDER[k + 6] == "GLCM_ASM"
    mask, order = featureset.expand(["ROI_RADIUS_MAX", "MEAN", "GLCM_ASM", "EULER_NUMBER"])
    assert mask == RR | E | _abi.FAM_INTENSITY | _abi.FAM_GLCM
    assert order == ["MEAN", "EULER_NUMBER", "ROI_RADIUS_MAX", "GLCM_ASM"]
    s = _abi.default_settings(64)
    names = _lib.column_names(mask, s)
    sel = featureset.column_selector(order, names, [0, 45, 90, 135])
    assert [names[j] for j in sel] == ["MEAN", "EULER_NUMBER", "ROI_RADIUS_MAX", "GLCM_ASM_0", "GLCM_ASM_45", "GLCM_ASM_90", "GLCM_ASM_135"]
    assert featureset.expand(["fract_dim_boxcount"]) == (F, ["FRACT_DIM_BOXCOUNT"])
    for unserved in ("PERIMETER", "CIRCULARITY", "EDGE_MEAN_INTENSITY", "CONVEX_HULL_AREA", "AREA_PIXELS_COUNT"):
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            featureset.expand([unserved])


@pytest.mark.parametrize("name", list(outline_cases.CASES))
def test_restatement_matches_the_reference_classes(name):
    b = outline_cases.batch(name)
    g = outline_cases.golden()[name]
    K = outline_ref.contours_of(b)
    assert [len(k) for k in K] == list(g["n_contour"])
    got = outline_ref.outline_table(b, K)
    bad = outline_cases.mismatches(got, g["table"], parity.REL_TOL)
    assert not bad, "\n".join(bad[:10])
    # the shifted-grid box counts of the small ROIs, scale by scale
    off = np.asarray(b.px_offset).astype(np.int64)
    checked = 0
    for r in range(b.n_roi):
        x, y = b.x[off[r]:off[r + 1]].astype(np.int64), b.y[off[r]:off[r + 1]].astype(np.int64)
        w, h = int(b.bbox_w[r]), int(b.bbox_h[r])
        if outline_ref.ceil_pow2(max(w, h)) > 32 or len(x) < 2:
            assert (g["box_counts"][r] == -1).all()
            continue
        for s_, counts in outline_ref.box_counts(x, y, w, h):
            assert list(g["box_counts"][r][5 - s_.bit_length() + 1]) == counts, (r, s_)
            checked += 1
    print(f"{name}: {b.n_roi} ROIs, {checked} box-count rows")
