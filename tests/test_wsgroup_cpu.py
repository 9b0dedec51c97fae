"""The whole-slide group (nyxhip_wsgroup_slides, nyxus_amd.NyxusWholeSlide), the parts that need no GPU: symbols, constants and the
column catalogue, the group *WHOLESLIDE*, the refusals of the older classes and of the new one, the radial-without-contour zeros, and the
numpy restatement tests/wsgroup_ref.py pinned to the reference's tables (tests/golden/wsgroup)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset, featureset_allmorph, featureset_morph, nyxus_wholeslide
from tests import parity, synth
from tests import wsgroup_cases as wc
from tests import wsgroup_ref as wr
from tests.wholeslide_cases import slide, slide_batch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = wc.golden()
S8 = _abi.default_settings(8)


def test_symbols_and_constants():
    lib = _lib.load()
    for sym in ("nyxhip_wsgroup_n_columns", "nyxhip_wsgroup_column_name", "nyxhip_wsgroup_slides"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(lib, sym)
    assert (_abi.WS_CONTOUR, _abi.WS_SMOMS, _abi.WS_IMOMS, _abi.WS_RADIAL, _abi.WS_ALL) == (1, 2, 4, 8, 15)
    assert _abi.WS_BAND_PIXELS == 16384 and _abi.FAM_WHOLE_SLIDE == 0x3FF
    assert hasattr(nyxus_amd, "NyxusWholeSlide") and issubclass(nyxus_amd.NyxusWholeSlide, nyxus_amd.NyxusAllMorphology)


def test_column_catalogue_of_every_mask():
    lib = _lib.load()
    alone = {_abi.WS_CONTOUR: _lib.morph_column_names(_abi.MORPH_CONTOUR), _abi.WS_SMOMS: _lib.column_names(_abi.FAM_SMOMS, S8),
             _abi.WS_IMOMS: _lib.column_names(_abi.FAM_IMOMS, S8), _abi.WS_RADIAL: _lib.column_names(_abi.FAM_RADIAL, S8)}
    assert [len(alone[b]) for b in (1, 2, 4, 8)] == [7, 90, 90, 24] == [_abi.WS_COLS[b] for b in (1, 2, 4, 8)]
    assert alone[_abi.WS_CONTOUR] == featureset_morph.CONTOUR
    for m in range(1, 16):
        want = [n for b in (1, 2, 4, 8) if m & b for n in alone[b]]          # blocks in the order of the bits
        assert lib.nyxhip_wsgroup_n_columns(m) == len(want)
        assert _lib.wsgroup_column_names(m) == want
        sl = [wr.block_slice(m, b) for b in (1, 2, 4, 8) if m & b]
        assert sl[0].start == 0 and sl[-1].stop == len(want)
    buf = C.create_string_buffer(64)
    for m in (0, 16, 17, 1 << 31):
        assert lib.nyxhip_wsgroup_n_columns(m) == -1
        assert lib.nyxhip_wsgroup_column_name(m, 0, buf, 64) == 1
    assert lib.nyxhip_wsgroup_column_name(1, 7, buf, 64) == 1 and lib.nyxhip_wsgroup_column_name(1, -1, buf, 64) == 1
    assert lib.nyxhip_wsgroup_column_name(15, 210, buf, 64) == 0 and buf.value == b"RADIAL_CV_7"
    assert lib.nyxhip_wsgroup_column_name(15, 211, buf, 64) == 1


def test_invalid_arguments_need_no_device():
    lib = _lib.load()
    img = slide(8, 4, np.uint16)
    out = np.zeros(256)
    t = _abi.Tiles()
    t.inten = img.ctypes.data; t.inten_dtype = _abi.U16; t.width = 8; t.height = 4; t.n_tiles = 1; t.memory = _abi.MEM_HOST
    assert lib.nyxhip_wsgroup_slides(None, C.byref(t), 15, C.byref(S8), out.ctypes.data, 256) == 1          # no context
    assert lib.nyxhip_wsgroup_slides(None, None, 15, C.byref(S8), out.ctypes.data, 256) == 1
    t.label = img.ctypes.data
    assert lib.nyxhip_wsgroup_slides(None, C.byref(t), 15, C.byref(S8), out.ctypes.data, 256) == 1          # a label image
    assert (out == 0).all()


def test_the_group_expands_to_the_twelve_classes():
    G = nyxus_wholeslide.WHOLESLIDE
    classes = nyxus_wholeslide.WHOLESLIDE_CLASSES
    assert list(classes) == ["ContourFeature", "PixelIntensityFeatures", "GLCMFeature", "GLDMFeature", "GLRLMFeature", "GLSZMFeature", "NGLDMfeature",
                             "NGTDMFeature", "GaborFeature", "Imoms2D_feature", "RadialDistributionFeature", "ZernikeFeature"]
    assert sorted(G) == sorted(c for v in classes.values() for c in v) and len(set(G)) == len(G)
    assert not set(G) & set(featureset.GLDZM) and not set(G) & set(featureset.SMOMS)
    order = featureset_allmorph.ALL_MORPH_REQUEST_ORDER
    assert [order.index(c) for c in G] == sorted(order.index(c) for c in G)                                 # enum order
    api = json.load(open(os.path.join(HERE, "golden", "wsgroup", "api_expected.json")))
    assert api["codes"] == G
    nyx = nyxus_amd.NyxusWholeSlide(["*WHOLESLIDE*"])
    assert nyx._requested == G
    # with label images the group is a plain expansion over entries that exist: the family mask, the contour bit of the morphology mask
    fam = 0
    for c in G:
        fam |= featureset.FAMILY_OF.get(c, 0)
    assert nyx._mask == fam and nyx._morph == _abi.MORPH_CONTOUR and not nyx._neighbors and not nyx._hexpoly
    cols, _ = nyx._columns()
    assert cols == api["columns"]
    assert nyx._ws_masks() == (_abi.WS_CONTOUR | _abi.WS_IMOMS | _abi.WS_RADIAL, False)


def test_the_older_classes_still_raise(tmp_path):
    for cls in (nyxus_amd.Nyxus, nyxus_amd.NyxusMorphology, nyxus_amd.NyxusAllMorphology):
        with pytest.raises(ValueError):
            cls(["*WHOLESLIDE*"])
    path = str(tmp_path / "absent.tif")
    for cls, code in ((nyxus_amd.Nyxus, "IMOM_WHU7"), (nyxus_amd.Nyxus, "SPAT_MOMENT_00"), (nyxus_amd.Nyxus, "FRAC_AT_D"),
                      (nyxus_amd.NyxusMorphology, "PERIMETER"), (nyxus_amd.NyxusAllMorphology, "PERIMETER"), (nyxus_amd.NyxusAllMorphology, "IMOM_WHU7")):
        nyx = cls(["MEAN", code])
        with pytest.raises(ValueError, match="whole-slide mode") as ei:
            nyx.featurize_files([path], None, True)
        assert code in str(ei.value) and nyx._ctx is None


@pytest.mark.parametrize("extra", ["CONVEX_HULL_AREA", "AREA_PIXELS_COUNT", "EXTREMA_P1_X", "NUM_NEIGHBORS", "IH_BIN_SIZE", "HEXAGONALITY_AVE", "GEODETIC_LENGTH",
                                   "EULER_NUMBER", "MAJOR_AXIS_LENGTH"])
def test_the_new_class_refuses_the_rest_before_a_context_is_made(extra, tmp_path):
    nyx = nyxus_amd.NyxusWholeSlide(["*WHOLESLIDE*", extra], ibsi=True)
    with pytest.raises(ValueError, match="whole-slide mode") as ei:
        nyx.featurize_files([str(tmp_path / "absent.tif")], None, True)
    named = str(ei.value).split("are not served")[0]
    assert extra in named and "PERIMETER" not in named and "IMOM_WHU7" not in named and "FRAC_AT_D" not in named and "MEAN" not in named
    assert nyx._ctx is None
    (tmp_path / "d").mkdir()
    with pytest.raises(ValueError, match="whole-slide mode"):
        nyx.featurize_directory(str(tmp_path / "d"))
    assert nyx._ctx is None


def test_radial_codes_without_a_contour_class_are_zeros_and_need_no_device(tmp_path):
    """reduce_trivial_rois.cpp:446-457: the reference builds the contour only for a contour-dependent class; the radial class is none."""
    p = str(tmp_path / "s.tif")
    synth.write_tiled_tiff(p, slide(33, 17, np.uint16), tile=16)
    nyx = nyxus_amd.NyxusWholeSlide(["RADIAL_CV", "FRAC_AT_D"])
    assert nyx._ws_masks() == (0, True)
    df = nyx.featurize_files([p, p], None, True)
    assert list(df.columns[4:]) == [f"FRAC_AT_D_{i}" for i in range(8)] + [f"RADIAL_CV_{i}" for i in range(8)]
    assert len(df) == 2 and (df.values[:, 4:].astype(float) == 0).all() and nyx._ctx is None
    # ... and with a contour or moment code the block is the device's
    assert nyxus_amd.NyxusWholeSlide(["RADIAL_CV", "PERIMETER"])._ws_masks() == (_abi.WS_CONTOUR | _abi.WS_RADIAL, False)
    assert nyxus_amd.NyxusWholeSlide(["MEAN_FRAC", "SPAT_MOMENT_00"])._ws_masks() == (_abi.WS_SMOMS | _abi.WS_RADIAL, False)
    assert nyxus_amd.NyxusWholeSlide(["MEAN", "MEAN_FRAC"])._ws_masks() == (0, True)


@pytest.mark.parametrize("name", list(wc.CASES))
def test_restatement_equals_the_recorded_reference(name):
    img = wc.image(name)
    want, got = GOLD[name + "__row"], wr.row(img)
    h, w = img.shape
    o, d2 = wr.centre(w, h)
    assert [d2, o % w, o // w] == [int(v) for v in GOLD[name + "__centre"]]
    assert np.array_equal(got[:7], want[:7]), name                                                          # the contour block, bit for bit
    if GOLD[name + "__radial_defined"]:
        assert np.array_equal(got[187:203], want[187:203]), name                                            # FRAC_AT_D / MEAN_FRAC, bit for bit
        bad = parity.compare_tables(got[None, 203:], want[None, 203:], _lib.wsgroup_column_names(_abi.WS_RADIAL)[16:])
        assert not bad, bad
    else:
        assert img.size == 1 and np.isnan(want[187:]).all() and (got[187:] == 0).all()                      # the ruling of DESIGN.md 4.5a
    names = _lib.wsgroup_column_names(_abi.WS_SMOMS | _abi.WS_IMOMS)
    bad = parity.compare_tables(got[None, 7:187], want[None, 7:187], names, batch=slide_batch([img]))
    assert not bad, bad[:8]
    assert np.array_equal(np.isnan(got[:187]), np.isnan(want[:187])) and np.array_equal(np.isinf(got[:187]), np.isinf(want[:187]))
    assert (name in wc.NAN_CASES) == bool((~np.isfinite(want[:187])).any())


def test_the_cases_cover_the_band_cut():
    from_plan = {n: -(-wc.CASES[n][1] // max(1, _abi.WS_BAND_PIXELS // wc.CASES[n][0])) for n in wc.CASES}
    assert (from_plan["b_exact"], from_plan["b_minus"], from_plan["b_plus"], from_plan["b_three"]) == (1, 1, 2, 3)
    assert wc.CASES["b_exact"][0] * wc.CASES["b_exact"][1] == _abi.WS_BAND_PIXELS
    assert wc.image("m33x257").max() > 1 << 31 and wc.image("m259x127").size % 2 == 1
