"""The 2-D morphology entries without a GPU: the constants and the column catalogue of every mask, the feature-code module and class
NyxusMorphology, and the restatement tests/morph_ref.py against values recorded from the reference's own classes
(tests/golden/morph): bit for bit, except the three columns the reference forms with an on-line update, which are held to
parity.REL_TOL / 10 against exact rationals."""
import itertools
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset, featureset_morph
from tests import morph_cases, morph_ref, parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = morph_cases.golden()
N = morph_ref.NAMES
MASKS = list(range(1, 16))
_REF = {}


def ref_table(name):
    """The restatement's table of a case, computed once and shared."""
    if name not in _REF:
        _REF[name] = morph_ref.table(morph_cases.batch(name))
    return _REF[name]


def test_constants_and_symbols():
    assert (_abi.MORPH_BASIC, _abi.MORPH_CONTOUR, _abi.MORPH_HULL, _abi.MORPH_EXTREMA, _abi.MORPH_ALL) == (1, 2, 4, 8, 15)
    hdr = open(os.path.join(ROOT, "include", "nyxhip.h")).read()
    for sym in ("nyxhip_morph_n_columns", "nyxhip_morph_column_name", "nyxhip_morph_batch", "nyxhip_morph_tiles"):
        assert sym in _lib.ABI_SYMBOLS and sym + "(" in hdr, sym
    for text in ("NYXHIP_MORPH_BASIC = 1u << 0", "NYXHIP_MORPH_CONTOUR = 1u << 1", "NYXHIP_MORPH_HULL = 1u << 2", "NYXHIP_MORPH_EXTREMA = 1u << 3",
                 "NYXHIP_MORPH_ALL = 0xFu", "#define NYXHIP_ABI_VERSION 2"):
        assert text in hdr, text
    lib = _lib.load()
    assert lib.nyxhip_abi_version() == 2


def test_column_catalogue_of_every_mask():
    assert _lib.morph_column_names(_abi.MORPH_ALL) == N and len(N) == 41
    assert [len(morph_ref.BLOCKS[b]) for b in (1, 2, 4, 8)] == [15, 7, 3, 16] == [_abi.MORPH_COLS[b] for b in (1, 2, 4, 8)]
    lib = _lib.load()
    for m in MASKS:
        names = _lib.morph_column_names(m)
        assert names == morph_ref.names_of(m) and lib.nyxhip_morph_n_columns(m) == len(names), m   # the other bits' names and order are kept
    assert N[N.index("EDGE_INTEGRATED_INTENSITY") + 1] == "CIRCULARITY" and N[N.index("CIRCULARITY") + 1] == "CONVEX_HULL_AREA"
    assert N == featureset_morph.ALL_MORPH


def test_bad_masks_and_columns_are_refused():
    import ctypes as C
    lib = _lib.load()
    buf = C.create_string_buffer(64)
    for m in (0, 16, 0x10 | 1, 1 << 31, 0xFFFFFFFF):
        assert lib.nyxhip_morph_n_columns(m) == -1
        assert lib.nyxhip_morph_column_name(m, 0, buf, 64) == 1
        with pytest.raises(_lib.NyxHipError):
            _lib.morph_column_names(m)
    assert lib.nyxhip_morph_column_name(1, 15, buf, 64) == 1 and lib.nyxhip_morph_column_name(1, -1, buf, 64) == 1
    assert lib.nyxhip_morph_column_name(15, 40, buf, 64) == 0 and buf.value == b"EXTREMA_P8_Y"
    assert lib.nyxhip_morph_column_name(15, 0, None, 64) == 1 and lib.nyxhip_morph_column_name(15, 0, buf, 0) == 1


def test_expand_morph_order_and_masks():
    M = featureset_morph
    assert len(M.MORPH_OF) == 41 and set(M.MORPH_OF.values()) == {1, 2, 4, 8}
    O = M.MORPH_REQUEST_ORDER
    assert len(O) == len(featureset.IH_REQUEST_ORDER) + 41 and [c for c in O if c not in M.MORPH_OF] == featureset.IH_REQUEST_ORDER
    assert O[O.index("ASPECT_RATIO") + 1] == "MAJOR_AXIS_LENGTH" and O[O.index("AREA_PIXELS_COUNT") - 1] == featureset.INTENSITY[-1]
    assert O[O.index("ROUNDNESS") + 1] == "PERIMETER" and O[O.index("SOLIDITY") + 1] == "EROSIONS_2_VANISH"
    assert O[O.index("EULER_NUMBER") + 1] == "EXTREMA_P1_X" and O[O.index("EXTREMA_P8_Y") + 1] == "DIAMETER_MIN_ENCLOSING_CIRCLE"
    assert M.expand_morph(["PERIMETER"]) == (0, 2, ["PERIMETER"])
    assert M.expand_morph(["solidity ", "AREA_PIXELS_COUNT"]) == (0, 5, ["AREA_PIXELS_COUNT", "SOLIDITY"])
    assert M.expand_morph(["*BASIC_MORPHOLOGY*"]) == (0, 1, M.BASIC)
    fam, mm, codes = M.expand_morph(["GLCM_ASM", "EXTREMA_P1_X", "NUM_NEIGHBORS", "EULER_NUMBER", "CIRCULARITY", "ROUNDNESS", "AREA_PIXELS_COUNT", "MEAN"])
    assert codes == ["MEAN", "AREA_PIXELS_COUNT", "ROUNDNESS", "CIRCULARITY", "EULER_NUMBER", "EXTREMA_P1_X", "NUM_NEIGHBORS", "GLCM_ASM"]
    assert mm == 1 | 4 | 8 and fam == featureset.expand(["GLCM_ASM", "NUM_NEIGHBORS", "EULER_NUMBER", "ROUNDNESS", "MEAN"])[0]
    assert M.expand_morph(["MEAN"]) == (featureset.expand(["MEAN"])[0], 0, ["MEAN"])
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        M.expand_morph(["PERIMETER", "POLYGONALITY_AVE"])
    with pytest.raises(ValueError, match="no features requested"):
        M.expand_morph([])
    with pytest.raises(ValueError) as ei:
        M.expand_morph(["*ALL_MORPHOLOGY*"])
    for code in ("POLYGONALITY_AVE", "HEXAGONALITY_AVE", "HEXAGONALITY_STDDEV"):
        assert code in str(ei.value)


def test_featureset_and_nyxus_still_refuse_the_codes():
    for code in N + ["*BASIC_MORPHOLOGY*", "*ALL_MORPHOLOGY*"]:
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            featureset.expand([code])
        assert code not in featureset.FAMILY_OF and code not in featureset.GROUPS
    for code in ("PERIMETER", "CONVEX_HULL_AREA", "AREA_PIXELS_COUNT", "*BASIC_MORPHOLOGY*"):
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            nyxus_amd.Nyxus([code])


def test_nyxus_morphology_constructs():
    nyx = nyxus_amd.NyxusMorphology(["PERIMETER", "MEAN", "*BASIC_MORPHOLOGY*"])
    assert isinstance(nyx, nyxus_amd.Nyxus) and nyx._morph == 3 and nyx._mask == _abi.FAM_INTENSITY and not nyx._neighbors and not nyx._ih
    assert nyx._requested == ["MEAN"] + featureset_morph.BASIC + ["PERIMETER"]
    only = nyxus_amd.NyxusMorphology(["EXTREMA_P4_Y"])
    assert only._morph == 8 and only._mask == 0 and only._active() == (["EXTREMA_P4_Y"], False)
    plain = nyxus_amd.NyxusMorphology(["MEAN"])
    assert plain._morph == 0 and plain._mask == _abi.FAM_INTENSITY
    nyx.set_environment_params(features=["SOLIDITY"])
    assert nyx._morph == 4 and nyx._mask == 0
    with pytest.raises(ValueError, match="HEXAGONALITY_STDDEV"):
        nyxus_amd.NyxusMorphology(["*ALL_MORPHOLOGY*"])
    with pytest.raises(ValueError, match="not served in whole-slide mode") as ei:
        nyxus_amd.NyxusMorphology(["MEAN", "PERIMETER"]).featurize_files(["a.tif"], None, single_roi=True)
    assert "PERIMETER" in str(ei.value) and "MEAN" not in str(ei.value).split("are not served")[0]


@pytest.mark.parametrize("name", list(morph_cases.CASES))
def test_restatement_equals_the_recorded_reference(name):
    want, R = GOLD[name]["table"], ref_table(name)
    assert want.shape == R.shape == (morph_cases.batch(name).n_roi, 41)
    rounded = [N.index(c) for c in morph_ref.ROUNDED]
    exact = [i for i in range(41) if i not in rounded]
    bad = want[:, exact].view(np.uint64) != R[:, exact].view(np.uint64)
    assert not bad.any(), [(int(r), N[exact[c]], want[r, exact[c]], R[r, exact[c]]) for r, c in np.argwhere(bad)[:8]]
    for c in rounded:
        assert (np.abs(R[:, c] - want[:, c]) <= parity.REL_TOL / 10 * np.abs(want[:, c])).all(), N[c]


def test_named_branches():
    c = {k: i for i, k in enumerate(N)}
    for name in morph_cases.CASES:
        T, nk = GOLD[name]["table"], GOLD[name]["n_contour"]
        assert (T[:, c["AREA_UM2"]] == 0).all(), name                        # the XY resolution setting is never filled
        assert (np.isinf(T[:, c["CIRCULARITY"]]) == (nk == 0)).all() and np.isfinite(np.delete(T, c["CIRCULARITY"], axis=1)).all(), name
        assert (T[nk == 0][:, [c[k] for k in morph_ref.CONTOUR]] == 0).all(), name
    small, nk = GOLD["small"]["table"], GOLD["small"]["n_contour"]
    assert nk.tolist() == [0, 0, 3, 2, 3, 0]
    assert small[0, c["CONVEX_HULL_AREA"]] == 1.0 and small[0, c["SOLIDITY"]] == 1.0          # one pixel: the empty hull
    assert small[:, c["COMPACTNESS"]].tolist()[:2] == [0.0, 0.0] and small[3, c["EDGE_STDDEV_INTENSITY"]] == 0.0   # n <= 2
    assert small[:, c["CONVEX_HULL_AREA"]].tolist() == [1.0, 2.0, 3.0, 3.0, 4.0, 2.0]
    needles = GOLD["collinear"]["table"]
    assert (needles[:, c["CONVEX_HULL_AREA"]] == needles[:, c["AREA_PIXELS_COUNT"]]).all() and (needles[:, c["SOLIDITY"]] == 1.0).all()
    assert GOLD["long_comb"]["n_contour"][0] > morph_cases.CONTOUR_LDS
    shapes = GOLD["shapes"]["table"]
    assert shapes[8, c["WEIGHTED_CENTROID_X"]] == 0 and shapes[8, c["WEIGHTED_CENTROID_Y"]] == 0 and shapes[8, c["MASS_DISPLACEMENT"]] > 0   # sum I = 0
    assert shapes[7, c["EDGE_STDDEV_INTENSITY"]] == 0 and shapes[7, c["EDGE_MEAN_INTENSITY"]] == 7          # flat intensities: nothing is skipped
    assert shapes[9, c["EDGE_MAX_INTENSITY"]] >= 2 ** 31
    # position: the columns that read coordinate differences only are identical across the four placements, the others move by the origin
    P, k = GOLD["placed"]["table"], morph_cases.N_PLACED
    free = [c[n] for n in N if n not in morph_ref.POSITION and n not in morph_ref.CENTROID_BOUND]
    for p, (ox, oy) in enumerate(morph_cases.PLACEMENTS):
        blk = P[p * k:(p + 1) * k]
        assert (blk[:, free].view(np.uint64) == P[:k, free].view(np.uint64)).all(), p
        for n in morph_ref.CENTROID_BOUND:                                   # formed from the rounded absolute centroids: a few ulp of the coordinate
            assert (np.abs(blk[:, c[n]] - P[:k, c[n]]) <= morph_ref.CENTROID_ULPS * np.spacing(float(max(ox, oy, 1)))).all(), (p, n)
        for n in morph_ref.EXTREMA + ["BBOX_XMIN", "BBOX_YMIN"]:
            assert (blk[:, c[n]] - P[:k, c[n]] == (ox if n in morph_ref.POSITION_X else oy)).all(), (p, n)
    # extrema ties: P1 .. P8 of the octagon and of the diamond
    ties = GOLD["ties"]["table"][:, c["EXTREMA_P1_X"]:]
    assert ties[0].tolist() == [3, 0, 7, 0, 10, 3, 10, 5, 7, 8, 3, 8, 0, 5, 0, 3]
    assert ties[1].tolist() == [4, 0, 4, 0, 8, 4, 8, 4, 4, 8, 4, 8, 0, 4, 0, 4]


def test_every_subset_of_the_restatement_is_a_selection():
    for m, bits in ((m, [b for b in (1, 2, 4, 8) if m & b]) for m in MASKS):
        assert morph_ref.columns_of(m) == list(itertools.chain.from_iterable([N.index(n) for n in morph_ref.BLOCKS[b]] for b in bits))
