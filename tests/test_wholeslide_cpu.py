"""Whole-slide mode (nyxhip_featurize_slides, Nyxus.featurize_files(..., single_roi=True), featurize_directory without labels), the parts
that need no GPU: the symbol, argument checks that come before any device use, the equivalent batch of tests/wholeslide_cases.py, and
the refusals of the Python class."""
import ctypes as C

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset
from oracle import pyoracle as po
from tests import wholeslide_cases as wc


def test_the_library_exports_the_entry():
    lib = _lib.load()
    assert lib.nyxhip_abi_version() == 2
    assert "nyxhip_featurize_slides" in _lib.ABI_SYMBOLS and hasattr(lib, "nyxhip_featurize_slides")
    assert _abi.FAM_WHOLE_SLIDE == _abi.FAM_ALL & ~(_abi.FAM_SMOMS | _abi.FAM_IMOMS) == 0x3FF


def _tiles(img, label=None):
    t = _abi.Tiles()
    t.inten = img.ctypes.data; t.label = label
    t.inten_dtype = _abi.U16; t.label_dtype = _abi.U16
    t.width = img.shape[1]; t.height = img.shape[0]; t.n_tiles = 1; t.memory = _abi.MEM_HOST
    return t


def test_invalid_arguments_need_no_device():
    """Checked before the context is looked at: the call is made without one, and the message says which check spoke."""
    lib = _lib.load()
    img = wc.slide(8, 4, np.uint16)
    out = np.zeros(512)
    s = _abi.default_settings(64)
    good = _tiles(img)
    labelled = _tiles(img, img.ctypes.data)
    ncol = 512

    def call(t, mask, sp, o):
        rc = lib.nyxhip_featurize_slides(None, C.byref(t) if t is not None else None, mask, C.byref(sp) if sp is not None else None,
                                         o.ctypes.data if o is not None else None, ncol)
        return rc, (lib.nyxhip_last_error(None) or b"").decode()

    for args in ((None, 1, s, out), (good, 1, None, out), (good, 1, s, None)):
        rc, msg = call(*args)
        assert rc == 1 and "null slides / settings / out_table" in msg
    rc, msg = call(labelled, 1, s, out)
    assert rc == 1 and "label must be NULL" in msg
    rc, msg = call(good, 0, s, out)
    assert rc == 1 and "bad family mask" in msg
    for bit in (12, 14, 26, 27, 28, 29, 30, 31):
        rc, msg = call(good, (1 << bit) | 1, s, out)
        assert rc == 1 and "bad family mask" in msg, bit
    assert (out == 0).all()


def test_slide_batch_is_the_stated_batch():
    imgs = [wc.slide(7, 3, np.uint8, "zeros"), wc.slide(2, 5, np.uint16), wc.slide(4, 4, np.uint32, "range70000")]
    b = wc.slide_batch(imgs)
    assert b.n_roi == 3 and b.px_offset.tolist() == [0, 21, 31, 47] and (b.roi_label == 1).all()
    assert b.bbox_w.tolist() == [7, 2, 4] and b.bbox_h.tolist() == [3, 5, 4]
    for r, img in enumerate(imgs):
        o, e = int(b.px_offset[r]), int(b.px_offset[r + 1])
        h, w = img.shape
        i = np.arange(w * h)
        assert (b.x[o:e] == i % w).all() and (b.y[o:e] == i // w).all()
        assert (b.inten[o:e] == img.reshape(-1)).all() and b.inten.dtype == np.uint32
        assert (img[b.y[o:e], b.x[o:e]] == b.inten[o:e]).all()
        assert b.min_inten[r] == img.min() and b.max_inten[r] == img.max()
        assert b.slide_min[r] == float(img.min()) and b.slide_max[r] == float(img.max())
    assert b.min_inten[0] == 0 and b.max_inten[2] - b.min_inten[2] == 70000
    assert b.origin_x is None and b.image_offset is None


def test_the_restatement_covers_the_whole_range_of_a_slide():
    s = _abi.default_settings(64)
    names = _lib.column_names(_abi.FAM_INTENSITY, s)
    b = wc.slide_batch([wc.slide(9, 6, np.uint16), wc.slide(9, 6, np.uint8, "zeros")])
    T = po.oracle_featurize(b, _abi.FAM_INTENSITY, s)
    assert (T[:, names.index("COVERED_IMAGE_INTENSITY_RANGE")] == 1.0).all()
    assert (T[:, names.index("MIN")] == b.min_inten).all() and (T[:, names.index("MAX")] == b.max_inten).all()


def test_empty_file_lists_raise():
    nyx = nyxus_amd.Nyxus(["*ALL_INTENSITY*"])
    with pytest.raises(ValueError):
        nyx.featurize_files([], None, True)
    with pytest.raises((ValueError, IOError)):
        nyx.featurize_files(None, None, True)
    assert nyx._ctx is None


@pytest.mark.parametrize("extra", ["GEODETIC_LENGTH", "IMOM_WHU7", "SPAT_MOMENT_00", "NUM_NEIGHBORS", "FRAC_AT_D", "EULER_NUMBER"])
def test_codes_outside_the_mode_raise_before_a_context_is_made(extra, tmp_path):
    nyx = nyxus_amd.Nyxus(["*ALL_INTENSITY*", extra])
    path = str(tmp_path / "absent.tif")
    with pytest.raises(ValueError, match="whole-slide mode") as ei:
        nyx.featurize_files([path], None, True)
    assert extra in str(ei.value) and "MEAN" not in str(ei.value).split("are not served")[0]
    assert nyx._ctx is None
    (tmp_path / "d").mkdir()
    with pytest.raises(ValueError, match="whole-slide mode"):
        nyx.featurize_directory(str(tmp_path / "d"))
    with pytest.raises(ValueError, match="whole-slide mode"):
        nyx.featurize_directory(str(tmp_path / "d"), str(tmp_path / "d"))
    assert nyx._ctx is None


def test_intensity_histogram_codes_raise_with_and_without_ibsi(tmp_path):
    for kw in ({}, {"ibsi": True}):
        nyx = nyxus_amd.Nyxus(["MEAN", "IH_BIN_SIZE"], **kw)
        with pytest.raises(ValueError, match="whole-slide mode") as ei:
            nyx.featurize_files([str(tmp_path / "absent.tif")], None, True)
        assert "IH_BIN_SIZE" in str(ei.value) and nyx._ctx is None


def test_pinned_refusals_still_hold():
    for unserved in ("PERIMETER", "AREA_PIXELS_COUNT", "CONVEX_HULL_AREA", "EXTREMA_P1_X", "HEXAGONALITY_AVE", "POLYGONALITY_AVE", "HISTOGRAM"):
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            featureset.expand([unserved])
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            nyxus_amd.Nyxus([unserved])
    with pytest.raises(ValueError, match="anisotropy"):
        nyxus_amd.Nyxus(["MEAN"], anisotropy_x=2.0)
