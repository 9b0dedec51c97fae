"""The volume texture entries without a GPU (nyxhip_voltex_n_columns, nyxhip_voltex_column_name, nyxhip_featurize_volumes_tex): the
catalogue, the refusals that need no device, the NumPy restatement (tests/voltex_ref.py) against the values recorded from the reference's
own D3_GLDM_feature / D3_NGLDM_feature / D3_NGTDM_feature (tests/golden/voltex), the cases themselves, the `Nyxus3D` face, and the
sensitivity of the columns to one count of any integer table."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset, featureset3d
from tests import vol_cases, voltex_cases, voltex_edge_cases, voltex_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "voltex", "voltex_reference.npz"))
SEAM_TOL = 1e-10             # the bound of tests/test_voltex_gpu.py


def test_symbols_and_catalogue():
    lib = _lib.load()
    for sym in ("nyxhip_voltex_n_columns", "nyxhip_voltex_column_name", "nyxhip_featurize_volumes_tex"):
        assert hasattr(lib, sym) and sym in _lib.ABI_SYMBOLS
    assert lib.nyxhip_abi_version() == 2
    blocks = {_abi.VTEX_GLDM: featureset3d.GLDM_3D, _abi.VTEX_NGLDM: featureset3d.NGLDM_3D, _abi.VTEX_NGTDM: featureset3d.NGTDM_3D}
    assert [len(v) for v in blocks.values()] == [14, 19, 5]
    for m in range(1, 8):
        want = [c for bit, cols in blocks.items() if m & bit for c in cols]
        assert _lib.voltex_column_names(m) == want and lib.nyxhip_voltex_n_columns(m) == len(want)
    names = _lib.voltex_column_names(_abi.VTEX_ALL)
    assert names[0] == "3GLDM_SDE" and names[13] == "3GLDM_LDHGLE" and names[14] == "3NGLDM_LDE" and names[32] == "3NGLDM_DCENE"
    assert names.index("3NGLDM_DCP") + 1 == names.index("3NGLDM_GLM") and names[33:] == ["3NGTDM_COARSENESS", "3NGTDM_CONTRAST", "3NGTDM_BUSYNESS", "3NGTDM_COMPLEXITY", "3NGTDM_STRENGTH"]
    buf = C.create_string_buffer(64)
    for m in [0, 8, 9, 15, 16, 1 << 12, 1 << 31, 0xFFFFFFFF]:
        assert lib.nyxhip_voltex_n_columns(m) < 0 and lib.nyxhip_voltex_column_name(m, 0, buf, 64) == 1
        with pytest.raises(_lib.NyxHipError):
            _lib.voltex_column_names(m)
    assert lib.nyxhip_voltex_column_name(7, 38, buf, 64) == 1 and lib.nyxhip_voltex_column_name(7, -1, buf, 64) == 1
    assert lib.nyxhip_voltex_column_name(7, 0, None, 64) == 1
    assert C.sizeof(_abi.VolTexSettings) == 12 and (_abi.VOLTEX_MAX_LEVELS, _abi.VOLTEX_MAX_RADIUS, _abi.VTEX_ALL) == (128, 3, 7)


def test_the_other_catalogues_are_unchanged():
    s = _abi.default_settings(64)
    assert len(_lib.vol_column_names(_abi.VFAM_ALL, s)) == vol_cases.N_COL == 455 and _abi.VFAM_ALL == 3
    assert _lib.vol_column_names(_abi.VFAM_ALL, s) == vol_cases.column_names()
    assert _lib.load().nyxhip_vol_n_columns(4, C.byref(s)) < 0
    assert not any(n.startswith("3") for n in _lib.column_names(_abi.FAM_ALL, s))
    assert not any(k.upper().startswith("*3D") for k in featureset.GROUPS) if hasattr(featureset, "GROUPS") else True


def test_a_null_context_is_refused_before_any_device_call():
    b = voltex_cases.batch("boxes")
    s, t = voltex_cases.settings("radiomics")
    cb = b.c_struct()
    out = np.zeros((b.n_roi, 38))
    assert _lib.load().nyxhip_featurize_volumes_tex(None, C.byref(cb), 7, C.byref(s), C.byref(t), out.ctypes.data, 38) == 1


@pytest.mark.parametrize("bname,mode", voltex_cases.CASES)
def test_restatement_against_the_recording(bname, mode):
    b = voltex_cases.batch(bname)
    s, t = voltex_cases.settings(mode)
    want = GOLD[voltex_cases.case_name(bname, mode)]
    bad, rel = voltex_cases.compare(voltex_ref.table(b, s, t), want)
    assert not bad, bad[:10]
    ex = voltex_cases.rule_excluded(b, s, t)
    nonflat = (b.max_inten != b.min_inten) & (b.counts() > 0)
    assert ex.mean() <= 0.05 and not ex[nonflat].any()


def test_the_cases_hold_what_they_are_named_for():
    b = voltex_cases.batch("boxes")
    boxes = list(zip(b.bbox_w.tolist(), b.bbox_h.tolist(), b.bbox_d.tolist()))
    assert boxes[:4] == [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2)] and boxes[5] == (7, 5, 1)
    assert sum(min(x) < 3 for x in boxes) >= 7 and sum(min(x) >= 3 for x in boxes) >= 3          # NGLDM: boxes without / with an interior cell
    assert int((b.max_inten == b.min_inten).sum()) == 3                                         # the flat ROIs
    names = voltex_cases.column_names()
    G = {m: GOLD[voltex_cases.case_name("boxes", m)] for m in ("radiomics", "matlab", "ibsi", "cap", "softnan", "r0", "r2")}
    flat = b.max_inten == b.min_inten
    assert (G["softnan"][flat][:, :33] == -7.5).all() and (G["radiomics"][flat][:, :33] == 0.0).all()   # flat: GLDM and NGLDM assign soft_nan
    assert (G["softnan"][flat][:, 33:] == -7.5).all()                                                    # ... and NGTDM has fewer than two levels
    # radius 0: every NGTDM code of a non-flat ROI is NaN
    assert np.isnan(G["r0"][~flat][:, 33:]).all() and np.isfinite(G["radiomics"][4, 33:]).all()
    # a box without an interior cell: NGLDM divides 0 by 0 where it divides, DCP is 1
    dcp = names.index("3NGLDM_DCP")
    assert np.isnan(G["radiomics"][1, 14]) and G["radiomics"][1, dcp] == 1.0 and np.isfinite(G["radiomics"][6, 14:33]).all()
    # the two binning forms and IBSI mode differ; radius 2 differs from radius 1 where the box is larger than the cube
    assert not np.allclose(G["radiomics"][11], G["matlab"][11], equal_nan=True) and not np.allclose(G["radiomics"][11], G["ibsi"][11], equal_nan=True)
    assert not np.allclose(G["radiomics"][11, 33:], G["r2"][11, 33:])
    s, t = voltex_cases.settings("cap")
    assert t.gldm_grey_depth == 128 and t.ngtdm_grey_depth == -128 and s.grey_depth == 128
    # NGTDM's +1: IBSI levels are 0 .. max, so the largest level value of the over-cap batch would be cap + 2
    sizes = [int(c[1].bbox_w[r]) * int(c[1].bbox_h[r]) * int(c[1].bbox_d[r]) for c in voltex_edge_cases.cases()[:3] for r in range(c[1].n_roi)]
    W = voltex_edge_cases.CELLS_PER_WG
    assert sizes == [W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 2, 3 * W + 2]
    for name, eb, es, et in voltex_edge_cases.cases()[3:]:
        r = et.ngtdm_radius
        sides = set(eb.bbox_w.tolist()) | set(eb.bbox_h.tolist()) | set(eb.bbox_d.tolist())
        assert {r, r + 1, 2 * r, 2 * r + 1, 2 * r + 2} <= sides, name
        # every class of the radius occurs in the largest box of the case
        T = voltex_ref.tables(eb, 5, es, et)
        assert (T["ngtdm_s"].sum(axis=0) > 0).all() and len(T["ngtdm_nd"]) == (r + 1) ** 3, name


def test_expansion_and_column_order():
    m, req = featureset3d.expand3d(["*3D_GLDM*", "*3d_ngldm*", "*3D_NGTDM*", "*3D_GLCM*"])
    assert m == _abi.VFAM_GLCM and featureset3d.tex_mask(req) == 7
    assert req == featureset3d.GLCM_3D + featureset3d.GLDM_3D + featureset3d.NGLDM_3D + featureset3d.NGTDM_3D      # behind the GLCM
    m, req = featureset3d.expand3d(["3NGTDM_STRENGTH", "3GLDM_DE", "3MEAN"])
    assert m == _abi.VFAM_INTENSITY and req == ["3MEAN", "3GLDM_DE", "3NGTDM_STRENGTH"] and featureset3d.tex_mask(req) == _abi.VTEX_GLDM | _abi.VTEX_NGTDM
    assert featureset3d.expand3d(["*3D_NGLDM*"])[0] == 0 and featureset3d.tex_mask(featureset3d.expand3d(["*3D_GLCM*"])[1]) == 0
    for f in ("*3D_GLRLM*", "*3D_GLSZM*", "*3D_GLDZM*", "3GLDM_NOPE", "*3D_ALL*"):
        with pytest.raises(ValueError, match="3D_ALL_INTENSITY.*3D_GLCM"):
            featureset3d.expand3d([f])
    n = nyxus_amd.Nyxus3D(["*3D_GLDM*", "*3D_NGLDM*", "*3D_NGTDM*", "*3D_GLCM*"])
    assert n._mask == _abi.VFAM_GLCM and n._tex_mask == 7
    cols, sel = n._columns()
    assert cols == n._requested and len(sel) == 59 + 38 and sel[59:] == list(range(419, 419 + 38))
    n2 = nyxus_amd.Nyxus3D(["3NGLDM_DCP", "3NGTDM_BUSYNESS"])
    assert n2._mask == 0 and n2._columns() == (["3NGLDM_DCP", "3NGTDM_BUSYNESS"], [12, 19 + 2])


def test_metaparameters():
    n = nyxus_amd.Nyxus3D(["*3D_GLDM*"])
    assert [n.get_metaparam(k) for k in ("3gldm/greydepth", "3ngtdm/greydepth", "3ngtdm/radius")] == [0.0, 0.0, 0.0]   # the reference's defaults
    n.set_metaparam("3gldm/greydepth=-20")
    n.set_metaparam("3ngtdm/greydepth=64")
    n.set_metaparam("3ngtdm/radius=2")
    assert (n.get_metaparam("3gldm/greydepth"), n.get_metaparam("3ngtdm/greydepth"), n.get_metaparam("3ngtdm/radius")) == (-20.0, 64.0, 2.0)
    assert (n._tex_settings.gldm_grey_depth, n._tex_settings.ngtdm_grey_depth, n._tex_settings.ngtdm_radius) == (-20, 64, 2)
    with pytest.raises(ValueError, match=r'Invalid metaparameter value 3gldm/greydepth=x: error: cannot parse value "x" of 3gldm/greydepth: expecting an integer'):
        n.set_metaparam("3gldm/greydepth=x")
    for bad in ("3ngtdm/radius=0", "3ngtdm/radius=-1", "3ngtdm/radius=1.5"):
        with pytest.raises(ValueError, match="Invalid metaparameter value .*3ngtdm/radius: expecting a positive integer"):
            n.set_metaparam(bad)
    with pytest.raises(ValueError, match="Invalid metaparameter value"):
        n.set_metaparam("3gldm/greydepth")
    for key in ("3glcm/greydepth=5", "3glrlm/greydepth=5", "3gldm/radius=1"):
        with pytest.raises(ValueError, match="3gldm/greydepth.*3ngtdm/greydepth.*3ngtdm/radius"):
            n.set_metaparam(key)
    with pytest.raises(ValueError, match="3gldm/greydepth.*3ngtdm/greydepth.*3ngtdm/radius"):
        n.get_metaparam("3glcm/offset")
    assert n.get_metaparam("3ngtdm/radius") == 2.0                                             # a refused value changes nothing


def _perturbations(T):
    """(table key, index, delta) samples: a count that exists lowered and raised, and an empty entry next to one raised."""
    rng = np.random.default_rng(5)
    for key in ("gldm", "ngldm", "ngtdm_n", "ngtdm_s"):
        M = T[key]
        nz = np.argwhere(M > 0)
        picks = [tuple(nz[i]) for i in rng.choice(len(nz), size=min(4, len(nz)), replace=False)] + [tuple(nz[0]), tuple(nz[-1])]
        for idx in picks:
            yield key, idx, -1
            yield key, idx, +1


@pytest.mark.parametrize("case", voltex_edge_cases.cases() + [("seam", voltex_cases.batch("seam"), *voltex_cases.settings("rad64"))], ids=lambda c: c[0])
def test_one_count_of_any_table_moves_a_column(case):
    """A lost or doubled voxel cannot hide under SEAM_TOL: +-1 in one entry of any integer table moves at least one column by more than
    10 x SEAM_TOL relative."""
    name, b, s, t = case
    r = max(range(b.n_roi), key=lambda i: int(b.bbox_w[i]) * int(b.bbox_h[i]) * int(b.bbox_d[i]))   # the largest ROI: one count weighs least
    T = voltex_ref.tables(b, r, s, t)
    base = voltex_ref.columns(T, s, t)
    for key, idx, delta in _perturbations(T):
        P = dict(T)
        P[key] = T[key].copy()
        P[key][idx] += delta
        moved = voltex_ref.columns(P, s, t)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(moved - base) / np.abs(base)
        assert np.nanmax(np.where(np.isfinite(rel), rel, 0.0)) > 10 * SEAM_TOL, (name, key, idx, delta)
