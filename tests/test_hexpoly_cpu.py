"""The hexagonality / polygonality class (POLYGONALITY_AVE, HEXAGONALITY_AVE, HEXAGONALITY_STDDEV; nyxhip_hexpoly_batch /
nyxhip_hexpoly_tiles) and the group *ALL_MORPHOLOGY*, the parts that need no GPU: tests/hexpoly_ref.py against values recorded from the
reference's own class (tests/golden/hexpoly) bit for bit -- gates, NaN and infinities included --, the entries and their column names,
the feature-code module and class NyxusAllMorphology, and the older expansions and classes, which keep refusing."""
import ctypes as C
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset, featureset_allmorph, featureset_morph
from tests import hexpoly_cases as hc, hexpoly_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = hc.golden()
API = hc.api_expected()
H = featureset_allmorph.HEXPOLY


@pytest.mark.parametrize("name", list(GOLD))
def test_restatement_equals_the_recorded_reference(name):
    """Every recorded row -- the ROIs of every case and the synthetic sweep -- bit for bit, a NaN standing where a NaN stands."""
    X, want = GOLD[name]
    got = hr.closing_rows(X)
    assert got.shape == want.shape == (len(X), 3)
    bad = [r for r in range(len(X)) if not hr.same_bits(got[r], want[r])]
    assert not bad, [(r, X[r].tolist(), got[r].tolist(), want[r].tolist()) for r in bad[:5]]


@pytest.mark.parametrize("name", [n for n in hc.CASES if n != "beyond_table"] + ["beyond_table"])
def test_recorded_inputs_are_those_of_the_restatements(name):
    """The six inputs the fixture was recorded at are what neighbors_ref, morph_ref and caliper_ref give for the case today."""
    assert hr.same_bits(hr.inputs_of(hc.batch(name), hc.radius(name)), GOLD[name][0])


def test_named_branches_occur_in_the_recorded_data():
    X, T = GOLD["low_counts"]
    assert sorted(set(X[:, 2].tolist())) == [0, 1, 2] and (T == -1).all()                      # fewer than three neighbors
    X, T = GOLD["no_contour"]
    assert (X[:, 1] == 0).sum() == 2 and (T[X[:, 1] == 0] == -1).all()                         # no contour
    assert (X[:, 2] >= 3).sum() == 4 and (T[X[:, 2] >= 3] != -1).all() and (T[(X[:, 2] < 3)] == -1).all()
    X, T = GOLD["lattice"]
    assert sorted(set(X[:, 2].tolist())) == [3, 5, 8] and np.isfinite(T).all() and (T != -1).all()
    for nb in (3, 5, 8):                                                                       # POLYGONALITY_AVE follows the neighbor count
        assert len(set(T[X[:, 2] == nb, 0].tolist())) == 1
    X, T = GOLD["needle"]
    assert X[0, 0] == 9 and X[0, 2] == 5 and 0 < X[0, 5] < 2 and X[0, 6] == 8 and np.isfinite(T[0]).all() and T[0, 1] < 0
    X, T = GOLD["beyond_table"]
    assert X[0, 2] == 400 > hr.TAN_TABLE_CAP and (X[1:, 2] <= hr.TAN_TABLE_CAP).all() and (X[:, 1] > 0).all()
    X, T = GOLD["hex_discs"]
    b = hc.batch("hex_discs")
    mid = [int(np.nonzero(np.asarray(b.roi_label) == lab)[0][0]) for lab in hc.HEX_MIDDLE]
    assert (X[mid, 2] == 6).all() and T[mid, 1].min() > GOLD["lattice"][1][:, 1].max() and T[mid, 0].min() > 9.5
    X, T = GOLD["deferred"]
    assert X[0, 0] == 2200 and X[0, 2] >= 3 and X[4, 0] == 10000 > hc.MORPH_PLANE_LDS and X[4, 2] >= 3 and (T[[0, 4]] != -1).all()
    assert hc.batch("deferred").bbox_w[0] == 1100 > hc.CALIPER_COLS_LDS
    X, T = GOLD["three_images"]
    assert (X[:9, 2] == X[9:18, 2]).all() and hr.same_bits(T[:9], T[9:18])                     # the same boxes in two images: no neighbor across
    assert hc.FAR_X > 2 ** 24 and (GOLD["far"][0][:, :5] == GOLD["lattice"][0][:, :5]).all() and (GOLD["far"][1][:, 0] == GOLD["lattice"][1][:, 0]).all()
    X, T = GOLD["sweep"]
    assert len(X) == 2000
    for nb in (0, 1, 2, 3, 4, 5, 128, 129, 1000):
        assert (X[:, 2] == nb).any(), nb
    live = X[:, 2] >= 3
    gates = (X[:, 1] == 0) | (X[:, 4] == 0) | ~live
    assert ((T == -1).all(axis=1) == gates).all()
    assert (live & (X[:, 1] == 0)).any() and (live & (X[:, 4] == 0)).any()
    open_ = live & ~gates
    assert (open_ & (X[:, 5] == 0)).any() and (open_ & (X[:, 3] == 0)).any() and (open_ & (X[:, 0] >= 2 ** 31)).any()
    assert np.isnan(T[open_]).any() and np.isinf(T[open_]).any() and not np.isfinite(T[open_ & (X[:, 5] == 0)][:, 1:]).any()


def test_entries_and_names():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "nyxhip.h")).read()
    for sym in ("nyxhip_hexpoly_column_name", "nyxhip_hexpoly_batch", "nyxhip_hexpoly_tiles"):
        assert hasattr(lib, sym) and sym in _lib.ABI_SYMBOLS and sym + "(" in hdr, sym
    assert "#define NYXHIP_HEXPOLY_COLS 3" in hdr and "#define NYXHIP_ABI_VERSION 2" in hdr and lib.nyxhip_abi_version() == 2
    assert _abi.HEXPOLY_COLS == 3 == len(hr.NAMES)
    assert _lib.hexpoly_column_names() == hr.NAMES == H == API["columns"]
    buf = C.create_string_buffer(64)
    assert lib.nyxhip_hexpoly_column_name(-1, buf, 64) == 1 and lib.nyxhip_hexpoly_column_name(3, buf, 64) == 1
    assert lib.nyxhip_hexpoly_column_name(0, None, 64) == 1 and lib.nyxhip_hexpoly_column_name(0, buf, 0) == 1
    assert lib.nyxhip_hexpoly_column_name(2, buf, 64) == 0 and buf.value == b"HEXAGONALITY_STDDEV"
    for method in ("hexpoly_host", "hexpoly_device", "hexpoly_tiles_host"):
        assert hasattr(_lib.Context, method)


def test_argument_errors_without_a_device():
    """Without a context nothing can be reported but the code: NYXHIP_ERR_INVALID_ARG from both entries, before anything touches a device."""
    lib = _lib.load()
    s = _abi.default_settings(64)
    out = np.zeros(3)
    n = C.c_uint64(7)
    cb = hc.batch("low_counts").c_struct()
    assert lib.nyxhip_hexpoly_batch(None, C.byref(cb), None, None, None, 0, 5, C.byref(s), out.ctypes.data, 3) == 1
    assert lib.nyxhip_hexpoly_batch(None, None, None, None, None, 0, 0, None, None, 0) == 1
    t = _abi.Tiles()
    assert lib.nyxhip_hexpoly_tiles(None, C.byref(t), 5, C.byref(s), None, None, 0, None, 0, C.byref(n)) == 1
    assert lib.nyxhip_hexpoly_tiles(None, None, -1, None, None, None, 0, None, 0, None) == 1


def test_all_morphology_expands_to_the_108_codes_in_enum_order():
    A = featureset_allmorph
    assert list(A.ALL_MORPHOLOGY_CLASSES) == list(API["all_morphology_classes"])               # the sixteen classes of env_features.cpp:256-271
    for cls, codes in A.ALL_MORPHOLOGY_CLASSES.items():
        assert sorted(codes) == sorted(API["all_morphology_classes"][cls]), cls                # ... and their featureset members
    assert [len(c) for c in A.ALL_MORPHOLOGY_CLASSES.values()] == [15, 3, 7, 6, 2, 2, 9, 3, 6, 1, 16, 2, 8, 6, 6, 16]
    fam, mm, hexpoly, codes = A.expand_all_morph(["*ALL_MORPHOLOGY*"])
    assert len(codes) == 108 == len(set(codes)) and codes == API["all_morphology"]             # the order of the reference's Feature2D enum
    assert hexpoly and mm == _abi.MORPH_ALL
    assert fam == featureset.expand(featureset.CIRCLES + featureset.FRACTAL + featureset.GEODETIC + featureset.NEIGHBORS + featureset.ROI_RADIUS
                                    + featureset.ELLIPSE + featureset.EULER + featureset.EROSION + featureset.FERET + featureset.MARTIN
                                    + featureset.NASSENSTEIN + featureset.CHORDS)[0]
    k = codes.index("POLYGONALITY_AVE")
    assert codes[k - 1] == "EXTREMA_P8_Y" and codes[k:k + 3] == H and codes[k + 3] == "DIAMETER_MIN_ENCLOSING_CIRCLE"
    O = A.ALL_MORPH_REQUEST_ORDER
    assert [c for c in O if c not in H] == featureset_morph.MORPH_REQUEST_ORDER and len(O) == len(featureset_morph.MORPH_REQUEST_ORDER) + 3
    assert A.expand_all_morph(["hexagonality_ave "]) == (0, 0, True, ["HEXAGONALITY_AVE"])
    assert A.expand_all_morph(["PERIMETER"]) == (0, 2, False, ["PERIMETER"])                   # everything expand_morph takes
    assert A.expand_all_morph(["*BASIC_MORPHOLOGY*"])[3] == featureset_morph.BASIC
    fam, mm, hexpoly, codes = A.expand_all_morph(["GLCM_ASM", "PERIMETER", "HEXAGONALITY_AVE", "MEAN"])
    assert codes == ["MEAN", "PERIMETER", "HEXAGONALITY_AVE", "GLCM_ASM"] and mm == 2 and hexpoly and fam == _abi.FAM_INTENSITY | _abi.FAM_GLCM
    with pytest.raises(ValueError, match="no features requested"):
        A.expand_all_morph([])
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        A.expand_all_morph(["HEXAGONALITY_AVE", "SHARPNESS"])


def test_the_older_expansions_and_classes_still_refuse():
    for code in H + ["*ALL_MORPHOLOGY*"]:
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            featureset.expand([code])
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            featureset_morph.expand_morph(["PERIMETER", code])
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            nyxus_amd.Nyxus([code])
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            nyxus_amd.NyxusMorphology([code])
        assert code not in featureset.FAMILY_OF and code not in featureset.GROUPS and code not in featureset_morph.MORPH_OF
        assert code not in featureset_morph.GROUPS_MORPH
    with pytest.raises(ValueError) as ei:
        featureset_morph.expand_morph(["*ALL_MORPHOLOGY*"])
    assert all(code in str(ei.value) for code in H)


def test_nyxus_all_morphology_constructs_and_refuses_whole_slide_mode():
    nyx = nyxus_amd.NyxusAllMorphology(["*ALL_MORPHOLOGY*"], neighbor_distance=7)
    assert isinstance(nyx, nyxus_amd.NyxusMorphology) and nyx._hexpoly and nyx._morph == _abi.MORPH_ALL and nyx._neighbors and not nyx._ih
    assert nyx._requested == API["all_morphology"] and nyx._env["neighbor_distance"] == 7
    only = nyxus_amd.NyxusAllMorphology(["POLYGONALITY_AVE"])
    assert only._hexpoly and only._mask == 0 and only._morph == 0 and not only._neighbors and only._active() == (["POLYGONALITY_AVE"], False)
    plain = nyxus_amd.NyxusAllMorphology(["MEAN", "PERIMETER"])
    assert not plain._hexpoly and plain._morph == 2 and plain._mask == _abi.FAM_INTENSITY
    only.set_environment_params(features=["SOLIDITY"])
    assert not only._hexpoly and only._morph == 4
    with pytest.raises(ValueError, match="not served in whole-slide mode") as ei:
        nyxus_amd.NyxusAllMorphology(["MEAN", "HEXAGONALITY_STDDEV", "POLYGONALITY_AVE"]).featurize_files(["a.tif"], None, single_roi=True)
    head = str(ei.value).split("are not served")[0]
    assert "HEXAGONALITY_STDDEV" in head and "POLYGONALITY_AVE" in head and "MEAN" not in head
    with pytest.raises(ValueError, match="not served in whole-slide mode") as ei:
        nyxus_amd.NyxusAllMorphology(["*ALL_MORPHOLOGY*"]).featurize_files(["a.tif"], None, single_roi=True)
    assert all(code in str(ei.value) for code in H)
