"""Radial intensity distribution (NYXHIP_FAM_RADIAL: FRAC_AT_D, MEAN_FRAC, RADIAL_CV), the parts that need no GPU: the column
catalogue, the Python feature set, and tests/radial_ref.py pinned to tables recorded from the reference's own classes
(tests/golden/radial)."""
import itertools
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset
from tests import radial_cases, radial_ref

RADIAL_CODES = ("FRAC_AT_D", "MEAN_FRAC", "RADIAL_CV")
FAMILY_BITS = ["FAM_INTENSITY", "FAM_GLCM", "FAM_GLRLM", "FAM_GLSZM", "FAM_NGTDM", "FAM_GABOR", "FAM_ZERNIKE", "FAM_GLDZM", "FAM_GLDM",
               "FAM_NGLDM", "FAM_SMOMS", "FAM_IMOMS"]


def test_family_bit_and_column_count():
    s = _abi.default_settings(64)
    assert _abi.FAM_RADIAL == 1 << 13 and _abi.FAM_ALL == 0xFFF and _abi.FAM_NORTH_STAR == 0x7F
    lib = _lib.load()
    assert lib.nyxhip_abi_version() == 2
    assert lib.nyxhip_n_columns(_abi.FAM_RADIAL, s) == 24
    assert _lib.column_names(_abi.FAM_RADIAL, s) == radial_ref.NAMES
    assert lib.nyxhip_n_columns(_abi.FAM_ALL | _abi.FAM_RADIAL, s) == lib.nyxhip_n_columns(_abi.FAM_ALL, s) + 24


def test_columns_interleave_with_gabor_in_enum_order():
    s = _abi.default_settings(64)
    names = _lib.column_names(_abi.FAM_GABOR | _abi.FAM_ZERNIKE | _abi.FAM_RADIAL, s)
    assert names.index("FRAC_AT_D_7") + 1 == names.index("GABOR_0")
    assert names.index("GABOR_3") + 1 == names.index("MEAN_FRAC_0")
    assert names.index("MEAN_FRAC_7") + 1 == names.index("RADIAL_CV_0")
    assert names.index("RADIAL_CV_7") + 1 == names.index("ZERNIKE2D_Z0")
    full = _lib.column_names(_abi.FAM_ALL | _abi.FAM_RADIAL, s)
    assert full.index("NGTDM_STRENGTH") + 1 == full.index("FRAC_AT_D_0") and full.index("ZERNIKE2D_Z29") + 1 == full.index("SPAT_MOMENT_00")
    assert [n for n in full if not n.startswith(RADIAL_CODES)] == _lib.column_names(_abi.FAM_ALL, s)


def _expanded(code, s):
    """Column names of one feature code (output_2_buffer.cpp:316-445) for the default settings."""
    if code in featureset.GLCM_ANGLED:
        return [f"{code}_{a}" for a in (0, 45, 90, 135)]
    if code in featureset.GLRLM_ANGLED:
        return [f"{code}_{a}" for a in (0, 45, 90, 135)]
    if code == "GABOR":
        return [f"GABOR_{i}" for i in range(s.gabor_n_filters)]
    if code == "ZERNIKE2D":
        return [f"ZERNIKE2D_Z{i}" for i in range(30)]
    return [code]


def test_masks_without_the_new_bit_keep_their_columns():
    """Every pre-existing mask (all 4095 of them): the column list built from featureset.ENUM_ORDER minus the new codes."""
    s = _abi.default_settings(64)
    lib = _lib.load()
    per_family = {}
    for code in featureset.ENUM_ORDER:
        if code not in RADIAL_CODES:
            per_family.setdefault(featureset.FAMILY_OF[code], []).extend(_expanded(code, s))
    order = []                                   # families in the order their first code appears in the enum
    for code in featureset.ENUM_ORDER:
        f = featureset.FAMILY_OF[code]
        if code not in RADIAL_CODES and f not in order:
            order.append(f)
    assert sorted(order) == sorted(getattr(_abi, b) for b in FAMILY_BITS)
    # GLRLM's angled and averaged codes, like GLCM's, are contiguous in the enum: one block per family
    singles = {f: _lib.column_names(f, s) for f in order}
    for f in order:
        assert singles[f] == per_family[f], f
    for mask in range(1, 0x1000):
        want = sum(len(singles[f]) for f in order if mask & f)
        assert lib.nyxhip_n_columns(mask, s) == want, mask
    for mask in [0xFFF, 0x7F, 0xC00, 0x060, 0x455] + [1 << k for k in range(12)] + [a | b for a, b in itertools.combinations([1 << k for k in range(12)], 2)]:
        assert _lib.column_names(mask, s) == [n for f in order if mask & f for n in singles[f]], mask


def test_featureset_expand_and_selector():
    mask, order = featureset.expand(["FRAC_AT_D", "GABOR"])
    assert mask == _abi.FAM_RADIAL | _abi.FAM_GABOR and order == ["FRAC_AT_D", "GABOR"]
    mask, order = featureset.expand(["ZERNIKE2D", "RADIAL_CV", "MEAN", "MEAN_FRAC"])
    assert mask == _abi.FAM_RADIAL | _abi.FAM_ZERNIKE | _abi.FAM_INTENSITY and order == ["MEAN", "MEAN_FRAC", "RADIAL_CV", "ZERNIKE2D"]
    i = featureset.ENUM_ORDER.index
    assert i("NGTDM_STRENGTH") + 1 == i("FRAC_AT_D") and i("FRAC_AT_D") + 1 == i("GABOR") and i("GABOR") + 1 == i("MEAN_FRAC")
    assert i("MEAN_FRAC") + 1 == i("RADIAL_CV") and i("RADIAL_CV") + 1 == i("ZERNIKE2D")
    assert not any("RADIAL" in g or "FRAC" in g for g in featureset.GROUPS)          # the reference has no group token for the family
    s = _abi.default_settings(64)
    cols = _lib.column_names(mask, s)
    sel = featureset.column_selector(order, cols, [0, 45, 90, 135])
    assert [cols[k] for k in sel] == ["MEAN"] + [f"MEAN_FRAC_{k}" for k in range(8)] + [f"RADIAL_CV_{k}" for k in range(8)] + \
        [f"ZERNIKE2D_Z{k}" for k in range(30)]


def test_unserved_features_still_raise():
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["PERIMETER"])
    with pytest.raises(ValueError, match="not served by the MI355X path.*FRAC_AT_D"):
        featureset.expand(["FRAC_AT_D", "CONVEX_HULL_AREA"])
    nyxus_amd.Nyxus(["GABOR", "FRAC_AT_D"])                                          # constructing needs no GPU


def _kernel_limit(name):
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "nyxus_amd", "csrc", "roi_kernel.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, hdr).group(1))


def test_fixture_inputs_are_defined_in_the_reference():
    """No row may be skipped: the recorded centre radius is non-zero wherever a contour exists."""
    G = radial_cases.golden()
    for name, g in G.items():
        assert g["table"].shape == (radial_cases.batch(name).n_roi, 24) and np.isfinite(g["table"]).all(), name
        assert not (g["dst2"] == 0).any() and ((g["dst2"] < 0) == (g["n_contour"] == 0)).all(), name
        assert (g["table"][g["n_contour"] == 0] == 0).all(), name
    K_MOM_CONTOUR_LDS, K_MOM_PX_LDS = _kernel_limit("kMomContourLds"), _kernel_limit("kMomPxLds")
    assert (K_MOM_CONTOUR_LDS, K_MOM_PX_LDS) == (2048, 3072)
    hb = radial_cases.batch("heavy")
    assert G["heavy"]["n_contour"].max() > K_MOM_CONTOUR_LDS and np.diff(hb.px_offset.astype(np.int64)).max() > K_MOM_PX_LDS
    assert (G["special"]["n_contour"] == 0).any()


def test_reference_regression_vector():
    """The reference's own regression vector for the 8 x 8 shape2d ROI (tests/test_2d_radial_regression.h:20-33, |d| <= 1e-9)."""
    here = os.path.dirname(os.path.abspath(__file__))
    reg = json.load(open(os.path.join(here, "golden", "radial", "reference_regression.json")))
    want = np.array(reg["FRAC_AT_D"] + reg["MEAN_FRAC"] + reg["RADIAL_CV"])
    got = radial_ref.radial_table(radial_cases.batch("shape2d"))[0]
    assert np.abs(got - want).max() <= 1e-9


@pytest.mark.parametrize("name", list(radial_cases.CASES))
def test_radial_ref_matches_the_reference_classes_bit_for_bit(name):
    b = radial_cases.batch(name)
    g = radial_cases.golden()[name]
    K = radial_ref.contours_of(b)
    assert [len(k) for k in K] == list(g["n_contour"])
    T, D = radial_ref.radial_table(b, K, with_dst2=True)
    assert [(-1.0 if d is None else float(d)) for d in D] == list(g["dst2"])
    same = T == g["table"]
    assert same.all(), np.argwhere(~same)[:10]


def test_pixel_order_reaches_the_row_only_through_the_centre_tie_break():
    """A permutation of an ROI's pixels leaves the contour (hence every distance) alone; the row changes only if another
    pixel of the same max - min becomes the first one."""
    rois = radial_cases.CASES["rand_seed9_rmax25"]()[:12]
    b = _abi.batch_from_rois(rois)
    rng = np.random.default_rng(0)
    perm = []
    for r in rois:
        p = rng.permutation(len(r["x"]))
        perm.append(dict(x=r["x"][p], y=r["y"][p], inten=r["inten"][p]))
    b2 = _abi.batch_from_rois(perm)
    K = radial_ref.contours_of(b)
    K2 = radial_ref.contours_of(b2)
    assert all((a == c).all() for a, c in zip(K, K2))
    T, T2 = radial_ref.radial_table(b, K), radial_ref.radial_table(b2, K2)
    off = b.px_offset.astype(np.int64)
    for r in range(b.n_roi):
        x, y = b.x[off[r]:off[r + 1]].astype(np.int64), b.y[off[r]:off[r + 1]].astype(np.int64)
        if len(K[r]) == 0:
            continue
        dif = [radial_ref.max_sqdist(int(a), int(c), K[r]) - radial_ref.min_sqdist(int(a), int(c), K[r]) for a, c in zip(x, y)]
        if dif.count(min(dif)) == 1:
            assert (T[r] == T2[r]).all(), r
