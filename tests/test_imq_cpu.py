"""The image-quality class (FOCUS_SCORE, LOCAL_FOCUS_SCORE, MAX_SATURATION, MIN_SATURATION: nyxhip_imq_batch / _tiles / _slides and
nyxus_amd.ImageQuality), the parts that need no GPU: the symbols and column names through the library, tests/imq_ref.py against the
values recorded from the reference's own classes (tests/golden/imq) and against the values its tests publish, the tile enumeration rule,
and the expansion, refusals and constructor checks of the Python class."""
import ctypes as C

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset, imq
from tests import imq_cases, imq_ref, parity

GOLD = imq_cases.golden()


def test_symbols_and_column_names_through_the_library():
    lib = _lib.load()
    assert lib.nyxhip_abi_version() == 2
    for sym in ("nyxhip_imq_column_name", "nyxhip_imq_batch", "nyxhip_imq_tiles", "nyxhip_imq_slides"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(lib, sym)
    assert _abi.IMQ_COLS == 4
    assert _lib.imq_column_names() == imq_ref.NAMES == imq_cases.NAMES == imq.IMQ_FEATURES == ["FOCUS_SCORE", "LOCAL_FOCUS_SCORE", "MAX_SATURATION", "MIN_SATURATION"]
    buf = C.create_string_buffer(64)
    assert lib.nyxhip_imq_column_name(-1, buf, 64) == 1 and lib.nyxhip_imq_column_name(4, buf, 64) == 1 and lib.nyxhip_imq_column_name(0, None, 64) == 1
    for name in ("nyxhip_imq_batch", "nyxhip_imq_tiles", "nyxhip_imq_slides", "NYXHIP_IMQ_COLS 4"):
        assert name in open(_header()).read()


def _header():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nyxhip.h")


def test_the_family_mask_does_not_learn_the_class():
    s = _abi.default_settings(64)
    everything = _abi.FAM_ALL | _abi.FAM_RADIAL | 0x3FF8000
    assert not set(imq_ref.NAMES) & set(_lib.column_names(everything, s))
    for frozen in (featureset.ENUM_ORDER, featureset.OUTPUT_ORDER, featureset.SERVED_ORDER, featureset.CATALOGUE_ORDER, featureset.FULL_ORDER,
                   featureset.EXPAND_ORDER, featureset.REQUEST_ORDER, featureset.IH_REQUEST_ORDER):
        assert not (set(imq_ref.NAMES) | set(imq.IMQ_UNSERVED)) & set(frozen)
    assert "*ALL_IMQ*" not in featureset.GROUPS


@pytest.mark.parametrize("name", list(imq_cases.CASES) + ["tile", "slides"])
def test_restatement_against_the_recording(name):
    b = imq_cases.tile_batch() if name == "tile" else imq_cases.slide_batch(imq_cases.api_tiles()[0]) if name == "slides" else imq_cases.batch(name)
    R, T = imq_ref.table(b, imq_cases.settings()), GOLD[name]
    assert R.shape == T.shape == (b.n_roi, 4)
    assert imq_ref.same_bits(R[:, imq_ref.SATURATION], T[:, imq_ref.SATURATION]).all()
    assert (imq_ref.rel_diff(R[:, imq_ref.FOCUS], T[:, imq_ref.FOCUS]) <= parity.REL_TOL).all()
    assert int(b.bbox_w.min()) >= 2 and int(b.bbox_h.min()) >= 2             # nothing recorded has a side of 1


def test_restatement_and_recording_against_the_published_values():
    pub = imq_cases.published()
    P = np.asarray(pub["image"], np.uint32)
    assert P.shape == (12, 8) and int((P == 0).sum()) == 18
    row = imq_ref.row_of_plane(P, 0.0)
    for c, col in enumerate(imq_ref.NAMES):
        want = pub["expected"][col]
        assert abs(row[c] - want) <= 1e-12 * abs(want), col
        assert abs(GOLD["published"][0, c] - want) <= pub["rel_tol"] * abs(want), col
    assert row[2] == 16 / 96 and row[3] == 18 / 96
    assert imq_ref.same_bits(imq_ref.table(imq_cases.batch("published"), imq_cases.settings())[0], np.array(row)).all()   # the cloud form of the plane


def test_named_properties_of_the_cases():
    assert (GOLD["zeros"][0] == [0.0, 0.0, 1.0, 0.0]).all()                  # zero-valued pixels only: no Laplacian, MAX = 1, MIN = 0
    assert (GOLD["flat"][0, 2:] == [1.0, 0.0]).all() and GOLD["flat"][0, 0] > 0
    b = imq_cases.batch("shapes")                                            # the background decides min P
    for r in range(b.n_roi):
        n, area = int(b.bbox_w[r]) * int(b.bbox_h[r]), int(b.px_offset[r + 1] - b.px_offset[r])
        assert area < n and b.min_inten[r] > 0 and GOLD["shapes"][r, 3] == (n - area) / n
    assert int(imq_cases.batch("extreme").max_inten.max()) == 2 ** 32 - 1 and int(imq_cases.batch("extreme").min_inten.min()) == 0
    side1 = imq_ref.table(imq_cases.batch("side1"), imq_cases.settings())
    assert (side1[:, 1] == imq_cases.SOFT_NAN).all() and (side1[:, [0, 2, 3]] != imq_cases.SOFT_NAN).all()
    assert list(side1[0]) == [0.0, imq_cases.SOFT_NAN, 1.0, 0.0]             # 1 x 1: one cell, variance 0, min P == max P


@pytest.mark.parametrize("h", [2, 3, 4, 5])
@pytest.mark.parametrize("w", [2, 3, 4, 5])
def test_tile_enumeration_rule(h, w):
    M, N = h // 2, w // 2
    ys = [0] if h % 2 == 0 else [0, M]
    xs = [0] if w % 2 == 0 else [0, N]
    assert imq_ref.tile_origins(h, w) == [(y, x) for y in ys for x in xs]
    for y0, x0 in imq_ref.tile_origins(h, w):
        assert y0 + M <= h and x0 + N <= w


def test_tile_counts_the_issue_names():
    assert len(imq_ref.tile_origins(2, 2)) == 1 and len(imq_ref.tile_origins(3, 3)) == 4
    assert len(imq_ref.tile_origins(5, 4)) == 2 and len(imq_ref.tile_origins(4, 5)) == 2      # a 5 x 4 box, either way round
    with pytest.raises(ValueError):
        imq_ref.tile_origins(1, 5)


def test_expansion():
    assert imq.expand_imq(["*ALL_IMQ*"]) == imq_ref.NAMES == imq.expand_imq(["*all_imq*"]) == imq.expand_imq(["*All_Imq*"])
    assert imq.expand_imq(["MIN_SATURATION", "focus_score"]) == ["FOCUS_SCORE", "MIN_SATURATION"]
    assert imq.expand_imq(["LOCAL_FOCUS_SCORE", "*ALL_IMQ*"]) == imq_ref.NAMES
    for name, word in (("POWER_SPECTRUM_SLOPE", "power_spectrum.cpp"), ("SHARPNESS", "sharpness.cpp"), ("sharpness", "swap")):
        with pytest.raises(ValueError, match="not served") as ei:
            imq.expand_imq([name])
        assert word in str(ei.value)
        with pytest.raises(ValueError, match="not served"):
            nyxus_amd.ImageQuality(["FOCUS_SCORE", name])
    for other in ("MEAN", "*ALL_INTENSITY*", "GLCM_ASM", "PERIMETER", "IH_MEAN_VAL", "*ALL*", "NO_SUCH_FEATURE"):
        with pytest.raises(ValueError, match="Nyxus"):
            nyxus_amd.ImageQuality([other])
        with pytest.raises(ValueError, match="Nyxus"):
            nyxus_amd.ImageQuality(["FOCUS_SCORE", other])
    with pytest.raises(ValueError, match="no features requested"):
        nyxus_amd.ImageQuality([])


def test_nyxus_still_refuses_the_codes():
    for name in ("FOCUS_SCORE", "LOCAL_FOCUS_SCORE", "MAX_SATURATION", "MIN_SATURATION", "POWER_SPECTRUM_SLOPE", "SHARPNESS", "*ALL_IMQ*"):
        with pytest.raises(ValueError):
            nyxus_amd.Nyxus([name])
        with pytest.raises(ValueError):
            featureset.expand([name])


def test_constructor_validation_and_no_context(capsys):
    iq = nyxus_amd.ImageQuality(["*ALL_IMQ*"])
    assert iq.get_params("coarse_gray_depth") == {"coarse_gray_depth": 256}
    assert iq._requested == imq_ref.NAMES and iq._mask == 0 and not iq._neighbors and not iq._ih and iq._ctx is None
    assert iq._columns() == (imq_ref.NAMES, [0, 1, 2, 3])
    assert nyxus_amd.ImageQuality(["MAX_SATURATION", "FOCUS_SCORE"])._columns() == (["FOCUS_SCORE", "MAX_SATURATION"], [0, 2])
    assert nyxus_amd.ImageQuality(["FOCUS_SCORE"], coarse_gray_depth=64).get_params("coarse_gray_depth") == {"coarse_gray_depth": 64}
    for kw, text in (({"neighbor_distance": 0}, "Neighbor distance must be greater than zero."),
                     ({"pixels_per_micron": 0}, "Pixels per micron must be greater than zero."),
                     ({"coarse_gray_depth": 0}, "default=256"),
                     ({"n_feature_calc_threads": 0}, "There must be at least one feature calculation thread."),
                     ({"verbose": -1}, "verbosity must be non-negative"),
                     ({"anisotropy_x": 0}, "anisotropy_x must be positive"),
                     ({"anisotropy_y": -1.0}, "anisotropy_y must be positive")):
        with pytest.raises(ValueError, match=text):
            nyxus_amd.ImageQuality(["*ALL_IMQ*"], **kw)
    # the refusals of this package, with the wording of Nyxus
    for kw in ({"anisotropy_x": 2.0}, {"anisotropy_y": 0.5}):
        with pytest.raises(ValueError) as a:
            nyxus_amd.ImageQuality(["*ALL_IMQ*"], **kw)
        with pytest.raises(ValueError) as n:
            nyxus_amd.Nyxus(["MEAN"], **kw)
        assert str(a.value) == str(n.value)
    img = np.ones((4, 4), np.uint16)
    for ot in ("arrowipc", "parquet"):
        with pytest.raises(ValueError) as a:
            iq.featurize(img, img, output_type=ot)
        with pytest.raises(ValueError) as n:
            nyxus_amd.Nyxus(["MEAN"]).featurize(img, img, output_type=ot)
        assert str(a.value) == str(n.value)
        with pytest.raises(ValueError):
            iq.featurize_files(["a.tif"], None, True, output_type=ot)
    with pytest.raises(ValueError, match="same dimension"):
        iq.featurize(img, img[None])
    with pytest.raises(IOError):
        iq.featurize_directory("/no/such/directory")
    with pytest.raises(IOError):
        iq.featurize_files(["a.tif"], None, False)
    capsys.readouterr()
    nyxus_amd.ImageQuality(["*ALL_IMQ*"], no_such_keyword=1)
    assert "unexpected keyword argument" in capsys.readouterr().out
    assert iq._ctx is None                                                   # no refused call created a context
    iq.set_params(features=["MIN_SATURATION"])
    assert iq._requested == ["MIN_SATURATION"]
    with pytest.raises(ValueError, match="Nyxus"):
        iq.set_params(features=["MEAN"])
