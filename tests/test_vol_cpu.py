"""The volume entries without a GPU (nyxhip_vol_n_columns / nyxhip_vol_column_name / nyxhip_featurize_volumes, nyxus_amd.Nyxus3D): the ABI
version, the column catalogue of the volume mask, its invalid bits, the 2-D catalogue as it was, the NumPy restatement (tests/vol_ref.py)
against the values recorded from the reference's own classes (tests/golden/vol), and the Python class's construction, name expansion and
refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset3d
from tests import vol_cases, vol_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "vol", "vol_reference.npz")


def test_abi_version_and_symbols():
    lib = _lib.load()
    assert lib.nyxhip_abi_version() == 2
    for sym in ("nyxhip_vol_n_columns", "nyxhip_vol_column_name", "nyxhip_featurize_volumes"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(_abi.Batch3D) == 14 * 8 + 4 * 4 + 8      # 14 pointers / counts, memory + three extrema, the budget


def test_column_catalogue():
    s = _abi.default_settings(64)
    both = _lib.vol_column_names(_abi.VFAM_ALL, s)
    assert len(both) == vol_cases.N_COL == 36 + 30 * 13 + 29 == 455
    assert both == vol_cases.column_names()
    assert both[0] == "3COV" and both[35] == "3UNIFORMITY_PIU" and both[:36] == featureset3d.INTENSITY_3D
    # the GLCM block in enum order (ACOR before ASM), 13 directions per code, _AVE behind the angled block
    assert both[36:36 + 13] == [f"3GLCM_ACOR_{k}" for k in range(13)] and both[36 + 13] == "3GLCM_ASM_0"
    assert both[36 + 29 * 13:36 + 30 * 13] == [f"3GLCM_VARIANCE_{k}" for k in range(13)]
    assert both[36 + 390] == "3GLCM_ASM_AVE" and both[-1] == "3GLCM_SUMVARIANCE_AVE" and both[36 + 390:] == featureset3d.GLCM_3D_AVE
    assert "3GLCM_HOM2_AVE" not in both and len(set(both)) == len(both)
    assert _lib.vol_column_names(_abi.VFAM_INTENSITY, s) == both[:36]
    assert _lib.vol_column_names(_abi.VFAM_GLCM, s) == both[36:]
    lib = _lib.load()
    buf = C.create_string_buffer(64)
    assert lib.nyxhip_vol_column_name(_abi.VFAM_GLCM, C.byref(s), 419, buf, 64) == 1
    assert lib.nyxhip_vol_column_name(_abi.VFAM_GLCM, C.byref(s), -1, buf, 64) == 1


@pytest.mark.parametrize("mask", [0, 1 << 2, 1 << 3, 1 << 12, 1 << 31, _abi.VFAM_ALL | (1 << 2), 0xFFFFFFFF])
def test_invalid_bits_of_the_volume_mask(mask):
    lib = _lib.load()
    s = _abi.default_settings(64)
    buf = C.create_string_buffer(64)
    assert lib.nyxhip_vol_n_columns(mask, C.byref(s)) < 0
    assert lib.nyxhip_vol_column_name(mask, C.byref(s), 0, buf, 64) == 1     # NYXHIP_ERR_INVALID_ARG


def test_the_2d_catalogue_is_unchanged():
    s = _abi.default_settings(8)
    lib = _lib.load()
    assert lib.nyxhip_n_columns(_abi.FAM_INTENSITY, C.byref(s)) == 36
    assert lib.nyxhip_n_columns(_abi.FAM_INTENSITY | _abi.FAM_GLCM, C.byref(s)) == 36 + 30 * 4 + 29
    assert _lib.column_names(_abi.FAM_GLCM, s)[:2] == ["GLCM_ASM_0", "GLCM_ASM_45"]
    assert not any(n.startswith("3") for n in _lib.column_names(_abi.FAM_ALL, s))
    for bit in (12, 14, 26, 31):
        assert lib.nyxhip_n_columns(1 << bit, C.byref(s)) <= 0      # (no columns: the 2-D mask does not know the bit)


@pytest.mark.parametrize("bname,mode", vol_cases.CASES)
def test_restatement_against_the_recording(bname, mode):
    gold = np.load(GOLD)
    b, s = vol_cases.batch(bname), vol_cases.settings(mode)
    want = gold[vol_cases.case_name(bname, mode)]
    got = vol_ref.table(b, s)
    assert got.shape == want.shape == (b.n_roi, vol_cases.N_COL)
    bad, ri, rg = vol_cases.compare(got, want)
    print(f"{bname}/{mode}: largest relative difference intensity {ri:.3e}, GLCM {rg:.3e}")
    assert not bad, bad[:10]


def test_the_cases_hold_what_they_are_named_for():
    gold = np.load(GOLD)
    b = vol_cases.batch("boxes")
    boxes = list(zip(b.bbox_w, b.bbox_h, b.bbox_d))
    assert boxes[:6] == [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (2, 2, 2), (7, 5, 1)] and boxes[8] == (4, 3, 2)
    assert list(b.counts()[6:8]) == [26, 27] and (b.inten[b.px_offset[7]:b.px_offset[8]] == 0).sum() == 1
    T = gold["boxes__matlab"][:, 36:36 + 390].reshape(-1, 30, 13)
    blank = (T == 0.0).all(axis=1)                          # soft_nan = 0: a blank direction is 30 zeros
    assert blank[0].all()                                   # 1x1x1: no pair in any direction
    assert [list(np.flatnonzero(~blank[r])) for r in (1, 2, 3)] == [[4], [10], [12]]   # (1,0,0), (0,1,0), (0,0,1)
    assert list(np.flatnonzero(~blank[5])) == [1, 4, 7, 10]                              # the slab: every dz != 0 direction blank
    T7 = gold["boxes__softnan"][:, 36:36 + 390].reshape(-1, 30, 13)
    assert (T7[1][:, [0, 1, 2, 3]] == -7.5).all() and (T7[1][:, 4] != -7.5).any()
    cells = vol_cases.batch("seam").cells()
    assert sorted(cells) == [vol_cases.LDS_CELLS - 1, vol_cases.LDS_CELLS, vol_cases.LDS_CELLS + 1]
    assert vol_cases.batch("blob40").cells()[0] == 64000 > vol_cases.LDS_CELLS
    w = vol_cases.batch("wide")
    assert int(w.max_inten[0]) - int(w.min_inten[0]) >= 2 ** 15 and int(w.max_inten[1]) == 2 ** 32 - 1
    assert int(vol_cases.batch("over").max_inten[0]) == vol_cases.LEVEL_CAP + 1
    # radiomics binning with fewer distinct levels than bins; a level count exactly at the cap
    assert vol_cases.settings("radiomics").glcm_grey_depth == -20 and vol_cases.settings("cap_matlab").glcm_grey_depth == vol_cases.LEVEL_CAP
    # only flat ROIs are taken out of the comparison, and only their GLCM columns under radiomics binning
    ex = vol_cases.rule_excluded(b, vol_cases.settings("radiomics"))
    flat = b.max_inten == b.min_inten
    assert (ex[:, :36] == False).all() and (ex[:, 36:].all(axis=1) == flat).all() and not vol_cases.rule_excluded(b, vol_cases.settings("ibsi")).any()


def test_nyxus3d_construction_expansion_and_refusals():
    n = nyxus_amd.Nyxus3D(["*3D_ALL_INTENSITY*"])
    assert n._mask == _abi.VFAM_INTENSITY and n._requested == featureset3d.INTENSITY_3D
    n = nyxus_amd.Nyxus3D(["*3d_glcm*", "3MEAN"], coarse_gray_depth=32, ibsi=True)
    assert n._mask == _abi.VFAM_ALL and n._requested == ["3MEAN"] + featureset3d.GLCM_3D
    assert n._settings.glcm_grey_depth == 32 and n._settings.ibsi == 1 and n._settings.glcm_offset == 1 and n._settings.glcm_symmetric == 0
    cols, sel = nyxus_amd.Nyxus3D(["3GLCM_CONTRAST_AVE", "3GLCM_ACOR", "3P99"])._columns()
    names = vol_cases.column_names()
    assert cols == ["3P99", "3GLCM_ACOR", "3GLCM_CONTRAST_AVE"] and [names[i] for i in sel] == ["3P99", "3GLCM_ACOR_0", "3GLCM_CONTRAST_AVE"]
    for bad in (["*3D_ALL*"], ["3AREA"], ["3GLRLM_SRE"], ["MEAN"], ["*ALL_GLCM*"], ["3GLCM_HOM2_AVE"], ["*3D_GLCM*", "3VOXEL_VOLUME"]):
        with pytest.raises(ValueError, match="3D_ALL_INTENSITY.*3D_GLCM"):
            nyxus_amd.Nyxus3D(bad)
    for kw, msg in ((dict(neighbor_distance=0), "Neighbor distance must be greater than zero."), (dict(pixels_per_micron=0), "Pixels per micron"),
                    (dict(coarse_gray_depth=0), "Custom number of grayscale levels"), (dict(n_feature_calc_threads=0), "at least one feature calculation thread"),
                    (dict(verbose=-1), "verbosity must be non-negative"), (dict(anisotropy_z=0), "anisotropy_z must be positive"),
                    (dict(anisotropy_x=-1), "anisotropy_x must be positive"), (dict(anisotropy_z=2.0), "anisotropy is outside"),
                    (dict(anisotropy_y=0.5), "anisotropy is outside")):
        with pytest.raises(ValueError, match=msg):
            nyxus_amd.Nyxus3D(["3MEAN"], **kw)
    n = nyxus_amd.Nyxus3D(["3MEAN"])
    for call in (n.featurize_directory, n.featurize_files):
        with pytest.raises(NotImplementedError, match="NIfTI / DICOM / z-stack"):
            call("a", "b")
    with pytest.raises(ValueError, match="same dimension"):
        n.featurize(np.zeros((2, 2, 2), np.uint16), np.zeros((2, 2), np.uint16))


def test_the_2d_class_still_refuses_3d_codes():
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["3COV"])
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["*3D_GLCM*"])


def test_host_side_refusals_need_no_gpu_state():
    """A volume mask with foreign bits never reaches a device call (a NULL context is refused first)."""
    lib = _lib.load()
    s = _abi.default_settings(64)
    cb = vol_cases.batch("boxes").c_struct()
    out = np.zeros((12, 455))
    assert lib.nyxhip_featurize_volumes(None, C.byref(cb), _abi.VFAM_ALL, C.byref(s), out.ctypes.data, 455) == 1
