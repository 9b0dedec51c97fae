"""The IBSI intensity-histogram family (46 IH_* codes, nyxhip_ih_batch / nyxhip_ih_tiles), the parts that need no GPU: the column
catalogue through the library, the feature-set plumbing, and tests/ih_ref.py against values recorded from the reference's own class
(tests/golden/ih) and against the two tables the reference's tests publish."""
import ctypes as C

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset
from tests import ih_cases, ih_ref, parity

GOLD = ih_cases.golden()
UNASSIGNED = (12, 14, 26, 27, 28, 29, 30, 31)


def test_names_count_and_order_through_the_library():
    lib = _lib.load()
    assert lib.nyxhip_abi_version() == 2
    assert _abi.IH_COLS == 46 == len(ih_ref.NAMES) == len(set(ih_ref.NAMES))
    assert _lib.ih_column_names() == ih_ref.NAMES == featureset.IH
    assert ih_ref.NAMES[0] == "IH_MEAN_VAL" and ih_ref.NAMES[19] == "IH_ROBUST_MEAN_VAL" and ih_ref.NAMES[20] == "IH_MEAN_IDX"
    assert ih_ref.NAMES[38:] == ["IH_UNIFORMITY_IDX", "IH_MAX_GRADIENT", "IH_MAX_GRADIENT_IDX", "IH_MIN_GRADIENT", "IH_MIN_GRADIENT_IDX",
                                 "IH_ROBUST_MEAN_IDX", "IH_NUM_BINS", "IH_BIN_SIZE"]
    assert len(ih_ref.EXACT) == 44 and set(ih_ref.NAMES) - set(ih_ref.EXACT) == {"IH_ENTROPY_VAL", "IH_ENTROPY_IDX"}
    buf = C.create_string_buffer(64)
    assert lib.nyxhip_ih_column_name(-1, buf, 64) == 1 and lib.nyxhip_ih_column_name(46, buf, 64) == 1 and lib.nyxhip_ih_column_name(0, None, 64) == 1
    for sym in ("nyxhip_ih_column_name", "nyxhip_ih_batch", "nyxhip_ih_tiles"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(lib, sym)


def test_the_family_mask_does_not_learn_the_class():
    s = _abi.default_settings(64, True)
    everything = _abi.FAM_ALL | _abi.FAM_RADIAL | 0x3FF8000
    assert not any(n.startswith("IH_") for n in _lib.column_names(everything, s))
    for bit in UNASSIGNED:                                                   # the pinned invalid bits stay out of the catalogue
        assert _lib.column_names(1 << bit, s) == []
    assert featureset.FAM_IH == 1 << 33 and featureset.FAM_NEIGHBORS == 1 << 32
    assert featureset.split_neighbors(featureset.FAM_IH | _abi.FAM_GLCM) == (_abi.FAM_GLCM, False)
    assert featureset.split_neighbors(featureset.FAM_IH | featureset.FAM_NEIGHBORS | 1) == (1, True)
    assert featureset.split_ih(featureset.FAM_IH | 1) and not featureset.split_ih(featureset.FAM_NEIGHBORS | 0xFFFFFFFF)


def test_expand_groups_single_codes_and_order():
    assert featureset.GROUPS["*ALL_IH*"] == ih_ref.NAMES
    assert featureset.expand(["*ALL_IH*"]) == (featureset.FAM_IH, ih_ref.NAMES)
    assert featureset.expand(["*all_ih*"]) == (featureset.FAM_IH, ih_ref.NAMES)
    assert featureset.expand(["ih_bin_size"]) == (featureset.FAM_IH, ["IH_BIN_SIZE"])
    assert all(featureset.FAMILY_OF[n] == featureset.FAM_IH for n in ih_ref.NAMES)
    mask, order = featureset.expand(["IH_NUM_BINS", "IMOM_WHU7", "MEAN", "IH_MEAN_VAL", "NUM_NEIGHBORS", "GLCM_ASM", "THICKNESS"])
    assert mask == featureset.FAM_IH | featureset.FAM_NEIGHBORS | _abi.FAM_IMOMS | _abi.FAM_INTENSITY | _abi.FAM_GLCM | _abi.FAM_GEODETIC
    assert order == ["MEAN", "THICKNESS", "NUM_NEIGHBORS", "GLCM_ASM", "IMOM_WHU7", "IH_MEAN_VAL", "IH_NUM_BINS"]
    # the earlier order lists keep the codes they had; the new one ends with the family
    new = set(ih_ref.NAMES)
    for frozen in (featureset.ENUM_ORDER, featureset.OUTPUT_ORDER, featureset.SERVED_ORDER, featureset.CATALOGUE_ORDER, featureset.FULL_ORDER,
                   featureset.EXPAND_ORDER, featureset.REQUEST_ORDER):
        assert not new & set(frozen)
    assert featureset.IH_REQUEST_ORDER == featureset.REQUEST_ORDER + ih_ref.NAMES and featureset.REQUEST_ORDER[-1] == "IMOM_WHU7"
    names = _lib.column_names(_abi.FAM_INTENSITY, _abi.default_settings(64)) + _lib.ih_column_names()
    sel = featureset.column_selector(["MEAN", "IH_MEAN_VAL", "IH_BIN_SIZE"], names, [0, 45, 90, 135])
    assert [names[j] for j in sel] == ["MEAN", "IH_MEAN_VAL", "IH_BIN_SIZE"]


def test_pinned_refusals_still_hold():
    for unserved in ("PERIMETER", "CIRCULARITY", "EDGE_MEAN_INTENSITY", "CONVEX_HULL_AREA", "AREA_PIXELS_COUNT", "EXTREMA_P1_X", "HEXAGONALITY_AVE",
                     "POLYGONALITY_AVE", "HISTOGRAM"):
        with pytest.raises(ValueError, match="not served by the MI355X path") as ei:
            featureset.expand([unserved])
        text = str(ei.value)
        assert "FRAC_AT_D" in text and "MAXCHORDS" in text and "EROSIONS_2_VANISH" in text and "NUM_NEIGHBORS" in text and "*ALL_IH*" in text
        assert all(n in text for n in ih_ref.NAMES)
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            nyxus_amd.Nyxus([unserved])


def test_nyxus_constructs_with_and_without_ibsi():
    for kw in ({}, {"ibsi": True}, {"ibsi": True, "coarse_gray_depth": 6}):
        nyx = nyxus_amd.Nyxus(["*ALL_IH*", "MEAN"], **kw)
        assert nyx._ih and nyx._mask == _abi.FAM_INTENSITY and not nyx._neighbors
        req, ih = nyx._active()
        assert ih == bool(kw.get("ibsi")) and req == (["MEAN"] + ih_ref.NAMES if ih else ["MEAN"])
    nyx = nyxus_amd.Nyxus(["IH_BIN_SIZE"])
    assert nyx._mask == 0 and nyx._ih
    with pytest.raises(ValueError, match="no features requested"):           # ibsi off at call time: the codes are dropped, nothing is left
        nyx._active()
    nyx.set_params(ibsi=True)
    assert nyx._active() == (["IH_BIN_SIZE"], True)
    plain = nyxus_amd.Nyxus(["MEAN"], ibsi=True)
    assert not plain._ih and plain._active() == (["MEAN"], False)


@pytest.mark.parametrize("name", list(ih_cases.CASES) + ["tile"])
def test_restatement_matches_the_reference_class(name):
    """Bit for bit on ih_ref.EXACT, parity.REL_TOL on the two entropy columns; the bin counts as recorded."""
    if name == "tile":
        b, s = ih_cases.tile_batch(), ih_cases.settings("sizes")
        s.grey_depth = ih_cases.API_DEPTH
    else:
        b, s = ih_cases.batch(name), ih_cases.settings(name)
    g = GOLD[name]
    T = ih_ref.table(b, s)
    assert T.shape == g["table"].shape == (b.n_roi, 46)
    ex = [ih_ref.NAMES.index(c) for c in ih_ref.EXACT]
    ok = ih_ref.same(T[:, ex], g["table"][:, ex])
    assert ok.all(), [(r, ih_ref.EXACT[c], T[r, ex[c]], g["table"][r, ex[c]]) for r, c in np.argwhere(~ok)[:8]]
    for c in ih_ref.ENTROPY:
        a, w = T[:, ih_ref.NAMES.index(c)], g["table"][:, ih_ref.NAMES.index(c)]
        assert (np.abs(a - w) <= parity.REL_TOL * np.abs(w)).all(), c
    for r in range(b.n_roi):
        o, e = int(b.px_offset[r]), int(b.px_offset[r + 1])
        if len(g["counts"][r]):
            want = ih_ref.counts(b.inten[o:e], int(b.min_inten[r]), int(b.max_inten[r]), int(s.grey_depth))
            assert (want == g["counts"][r]).all() and want.sum() == e - o
        else:
            assert (g["table"][r] == s.soft_nan).all()


def test_the_two_published_tables():
    pub = ih_cases.published()
    for key, case in (("five_pixel", "five"), ("ibsi_phantom", "phantom")):
        p = pub[key]
        assert ih_cases.settings(case).grey_depth == p["grey_depth"]
        assert ih_cases.batch(case).inten.tolist() == p["intensities"]
        for row in (ih_ref.table(ih_cases.batch(case), ih_cases.settings(case))[0], GOLD[case]["table"][0]):
            for col, want in p["expected"].items():
                got = row[ih_ref.NAMES.index(col)]
                if want == 0:
                    assert abs(got) <= 1e-9, col
                else:
                    assert abs(got - want) <= p["rel_tol"] * abs(want), (key, col, got, want)
    assert len(pub["ibsi_phantom"]["intensities"]) == 74 and len(pub["ibsi_phantom"]["expected"]) == 12
    assert GOLD["five"]["counts"][0].tolist() == [2, 1, 2]


def test_named_values_and_quirks():
    N = ih_ref.NAMES.index
    five = GOLD["five"]["table"][0]
    assert same_bits(GOLD["five_softnan"]["table"][0], five)
    assert five[N("IH_ENTROPY_IDX")] == five[N("IH_ENTROPY_VAL")] and five[N("IH_UNIFORMITY_IDX")] == five[N("IH_UNIFORMITY_VAL")]
    for name in ("gates", "gate_negative_depth", "gate_ibsi_off"):
        assert (GOLD[name]["table"] == ih_cases.SOFT_NAN).all()
    ng = GOLD["no_gradient"]["table"]
    assert (ng[:2, N("IH_MAX_GRADIENT")] == ih_ref.DBL_MIN).all() and (ng[:2, N("IH_MAX_GRADIENT_IDX")] == 0).all()
    assert GOLD["flat_big"]["counts"][0].max() > 65535
    sizes = [len(c["inten"]) for c in ih_cases.CASES["sizes"]["rois"]()]
    assert sizes[:6] == [63, 64, 65, 255, 256, 257] and ih_cases.WAVE_PX == 256
    r = GOLD["ramp_n64"]["counts"]
    assert r[0].sum() == 2 and r[1].sum() == 1001 and r[2].sum() == 65536 and (r[2] == 1024).all()
    assert GOLD["ramp_n4096"]["counts"][0].sum() == 65536 and len(GOLD["ramp_n4096"]["counts"][0]) == ih_cases.N_CAP
    k = ih_cases.mixed_row("disks")
    assert ih_ref.same(GOLD["mixed"]["table"][k:k + 4], GOLD["disks"]["table"]).all()


def same_bits(a, b):
    return bool(ih_ref.same(a, b).all())
