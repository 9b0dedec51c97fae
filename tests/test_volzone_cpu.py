"""The volume zone entries without a GPU (nyxhip_volzone_n_columns, nyxhip_volzone_column_name, nyxhip_featurize_volumes_zones): the
catalogue, the refusals that need no device, the NumPy restatement (tests/volzone_ref.py) against the values recorded from the reference's
own D3_GLRLM_feature / D3_GLSZM_feature (tests/golden/volzone), the cases themselves, `expand3d_zones` and the `Nyxus3DZones` face, and
the sensitivity of the columns to one count of any integer matrix."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset3d
from tests import vol_cases, voltex_cases, volzone_cases, volzone_edge_cases, volzone_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "volzone", "volzone_reference.npz"))
SEAM_TOL = 1e-10             # the bound of tests/test_volzone_gpu.py
W = volzone_cases.W


def test_symbols_and_catalogue():
    lib = _lib.load()
    for sym in ("nyxhip_volzone_n_columns", "nyxhip_volzone_column_name", "nyxhip_featurize_volumes_zones"):
        assert hasattr(lib, sym) and sym in _lib.ABI_SYMBOLS
    assert lib.nyxhip_abi_version() == 2
    f3 = featureset3d
    rl = [f"{c}_{k}" for c in f3.GLRLM_3D_ANGLED for k in range(13)] + f3.GLRLM_3D_AVE
    blocks = {_abi.VZONE_GLRLM: rl, _abi.VZONE_GLSZM: f3.GLSZM_3D}
    assert [len(v) for v in blocks.values()] == [224, 16]
    for m in (1, 2, 3):
        want = [c for bit, cols in blocks.items() if m & bit for c in cols]
        assert _lib.volzone_column_names(m) == want and lib.nyxhip_volzone_n_columns(m) == len(want)
    names = _lib.volzone_column_names(_abi.VZONE_ALL)
    assert names == volzone_cases.column_names() and len(names) == volzone_cases.N_COL == 240
    assert names[0] == "3GLRLM_SRE_0" and names[12] == "3GLRLM_SRE_12" and names[13] == "3GLRLM_LRE_0" and names[207] == "3GLRLM_LRHGLE_12"
    assert names[208] == "3GLRLM_SRE_AVE" and names[223] == "3GLRLM_LRHGLE_AVE" and names[224] == "3GLSZM_SAE" and names[239] == "3GLSZM_LAHGLE"
    buf = C.create_string_buffer(64)
    for m in [0, 4, 5, 8, 1 << 31, 0xFFFFFFFF]:
        assert lib.nyxhip_volzone_n_columns(m) < 0 and lib.nyxhip_volzone_column_name(m, 0, buf, 64) == 1
        with pytest.raises(_lib.NyxHipError):
            _lib.volzone_column_names(m)
    assert lib.nyxhip_volzone_column_name(3, 240, buf, 64) == 1 and lib.nyxhip_volzone_column_name(3, -1, buf, 64) == 1
    assert lib.nyxhip_volzone_column_name(2, 16, buf, 64) == 1 and lib.nyxhip_volzone_column_name(3, 0, None, 64) == 1
    assert C.sizeof(_abi.VolZoneSettings) == 8 and (_abi.VOLZONE_MAX_LEVELS, _abi.VZONE_GLRLM, _abi.VZONE_GLSZM, _abi.VZONE_ALL) == (128, 1, 2, 3)
    assert volzone_ref.SHIFTS13[0] == (1, 1, 1) and volzone_ref.SHIFTS13[4] == (1, 0, 0) and volzone_ref.SHIFTS13[12] == (0, 0, 1)   # (dz, dy, dx)


def test_the_other_catalogues_are_unchanged():
    s = _abi.default_settings(64)
    assert _lib.vol_column_names(_abi.VFAM_ALL, s) == vol_cases.column_names() and _abi.VFAM_ALL == 3
    assert _lib.voltex_column_names(_abi.VTEX_ALL) == voltex_cases.column_names() and _abi.VTEX_ALL == 7
    assert _lib.load().nyxhip_vol_n_columns(4, C.byref(s)) < 0 and _lib.load().nyxhip_voltex_n_columns(8) < 0
    assert not any(n.startswith("3") for n in _lib.column_names(_abi.FAM_ALL, s))


def test_a_null_context_is_refused_before_any_device_call():
    b = volzone_cases.batch("boxes")
    s, t = volzone_cases.settings("radiomics")
    cb = b.c_struct()
    out = np.zeros((b.n_roi, 240))
    assert _lib.load().nyxhip_featurize_volumes_zones(None, C.byref(cb), 3, C.byref(s), C.byref(t), out.ctypes.data, 240) == 1


@pytest.mark.parametrize("bname,mode", volzone_cases.CASES)
def test_the_restatement_agrees_with_the_recording(bname, mode):
    b = volzone_cases.batch(bname)
    s, t = volzone_cases.settings(mode)
    want = GOLD[volzone_cases.case_name(bname, mode)]
    got = volzone_ref.table(b, s, t)
    assert got.shape == want.shape == (b.n_roi, 240)
    bad, rel = volzone_cases.compare(got, want)
    assert not bad, bad[:10]
    ex = volzone_cases.rule_excluded(b, s, t)
    assert ex.mean() <= 0.05 and (ex.any() == (bname == "rule"))
    flat = b.max_inten == b.min_inten
    assert (want[flat][:, :208] == s.soft_nan).all() and (want[flat][:, 224:] == s.soft_nan).all()      # flat ROIs: before any binning
    assert np.allclose(want[flat][:, 208:224], s.soft_nan, rtol=1e-15, atol=0)                          # the average of thirteen soft_nan


def test_the_cases_hold_what_they_are_named_for():
    s, t = volzone_cases.settings("none")
    b = volzone_cases.batch("boxes")
    assert int((b.max_inten == b.min_inten).sum()) >= 3 and b.max_inten.max() <= volzone_cases.LEVEL_CAP
    boxes = set(zip(b.bbox_w.tolist(), b.bbox_h.tolist(), b.bbox_d.tolist()))
    assert {(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (7, 5, 1), (3, 3, 3), (5, 4, 3), (12, 12, 12)} <= boxes
    # connectivity
    b = volzone_cases.batch("conn")
    for r, (zones7, runs7) in enumerate(volzone_cases.CONN_PAIRS):
        T = volzone_ref.tables(b, r, s, t)
        Z = T["zones"]
        assert int(Z[Z[:, 0] == 7, 2].sum()) == zones7, r
        assert int(T["glrlm"][0][7].sum()) == runs7, r
    corner = volzone_ref.tables(b, 0, s, t)["glrlm"]
    assert [int(M[7].sum()) for M in corner] == [1] + [2] * 12 and corner[0][7, 1] == 1       # one run of two cells along (1, 1, 1) only
    sm, tm = volzone_cases.settings("mat4")
    Tm = volzone_ref.tables(b, 4, sm, tm)                  # the ROI voxels of value 0 bin to level 1, the background level: no zone
    assert 1 in Tm["sz_levels"] and not (Tm["zones"][:, 0] == 1).any() and Tm["glrlm"][12][1].sum() > 0   # ... but they form runs
    assert volzone_ref.tables(b, 5, s, t)["zones"].tolist() == [[1, 864, 1], [2, 864, 1]]     # the checkerboard: exactly 2 zones
    single = volzone_ref.tables(b, 6, s, t)["zones"]
    assert (single[:, 1] == 1).all() and single[:, 2].sum() == 1728 and len(single) == 8
    # runs: per direction a full-length run, a broken one, one that ends at the far face
    b = volzone_cases.batch("runs")
    for k, sh in enumerate(volzone_ref.SHIFTS13):
        L = volzone_ref.dir_len(sh, 3, 4, 5)
        full, broken, face = (volzone_ref.tables(b, 3 * k + q, s, t)["glrlm"][k] for q in range(3))
        assert full[9, L - 1] == 1 and full[9].sum() == 1, k
        assert face[9, L - 2] == 1 and face[9].sum() == 1, k
        if L > 2:
            assert broken[9].sum() == 2 and broken[4, 0] >= 1 and broken[9, L - 1] == 0, k
    # adversaries
    b = volzone_cases.batch("snakes")
    Z = volzone_ref.tables(b, 0, s, t)["zones"]
    assert Z[Z[:, 0] == 5].tolist() == [[5, int((volzone_cases.serpentine(16) == 5).sum()), 1]]
    Z = volzone_ref.tables(b, 2, s, t)["zones"]
    assert Z[Z[:, 0] == 8].tolist() == [[8, 63, 1]]         # the two arms are one zone through the corner contacts
    # the rule cases
    b = volzone_cases.batch("rule")
    assert (b.bbox_w[0], b.bbox_h[0], b.bbox_d[0]) == (36, 36, 37) and volzone_ref.tables(b, 0, s, t)["zones"][:, 1].max() > 46340
    M = volzone_ref.tables(b, 1, s, t)["glrlm"][12]
    assert (b.bbox_w[1], b.bbox_h[1], b.bbox_d[1]) == (600, 1, 1) and M[128, 519] == 1 and 128 * 520 >= 1 << 16
    # seams, in terms of W
    assert volzone_edge_cases.CELLS_PER_WG == W == 4096
    cells = [int(w) * int(h) * int(d) for c in volzone_edge_cases.cases()[:3] for w, h, d in zip(c[1].bbox_w, c[1].bbox_h, c[1].bbox_d)]
    assert cells == [W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 2, 3 * W + 2]
    crossed = 0
    for name, b, s, t in volzone_edge_cases.cases()[:3]:
        for r in range(b.n_roi):
            V, n, _, _ = volzone_ref.cube(b, r)
            d, h, w = V.shape
            inside = np.zeros(V.shape, bool)
            o0, o1 = int(b.px_offset[r]), int(b.px_offset[r + 1])
            inside[b.z[o0:o1], b.y[o0:o1], b.x[o0:o1]] = True
            for c in range(W, V.size, W):                  # a 26-adjacent pair of one value inside the cloud: one zone, one run, two ranges
                p = volzone_edge_cases.earlier_neighbour(c, w, h, d)
                assert p < c and V.flat[p] == V.flat[c] != 0 and inside.flat[p] and inside.flat[c], (name, r, c)
                crossed += 1
    assert crossed == 0 + 0 + 1 + 1 + 1 + 2 + 3
    name, b, s, t = volzone_edge_cases.cases()[3]
    L = volzone_cases.LANES
    longest = [max(int(np.flatnonzero(M.sum(axis=0)).max()) + 1 for M in volzone_ref.tables(b, r, s, t)["glrlm"]) for r in range(9)]
    assert longest == [L - 1] * 3 + [L] * 3 + [L + 1] * 3
    assert [int(volzone_ref.tables(b, r, s, t)["zones"][:, 1].max()) for r in range(9)] == longest
    assert [int(volzone_ref.tables(b, 9 + q, s, t)["zones"][:, 2].sum()) for q in range(3)] == [L - 1, L, L + 1]
    name, b, s, t = volzone_edge_cases.cases()[4]
    sizes = set(volzone_ref.tables(b, 0, s, t)["zones"][:, 1].tolist())
    assert {volzone_cases.SHORT_RUNS - 1, volzone_cases.SHORT_RUNS, volzone_cases.SHORT_RUNS + 1, volzone_cases.DENSE_SIZES - 1, volzone_cases.DENSE_SIZES,
            volzone_cases.DENSE_SIZES + 1} <= sizes


def test_expansion_and_column_order():
    f3 = featureset3d
    assert (len(f3.GLRLM_3D_ANGLED), len(f3.GLRLM_3D_AVE), len(f3.GLSZM_3D)) == (16, 16, 16)
    assert set(f3.GROUPS_3D_ZONES) == {"*3D_GLRLM*", "*3D_GLSZM*"}
    # Feature3D order (featureset.h): ... GLDM, NGLDM, NGTDM, then the GLSZM block, then the GLRLM block
    assert f3.ORDER_3D_ZONES == f3.ORDER_3D + f3.GLSZM_3D + f3.GLRLM_3D_ANGLED + f3.GLRLM_3D_AVE
    mask, req = f3.expand3d_zones(["*3d_glrlm*", "3GLSZM_ZP", "*3D_NGTDM*", "3mean"])
    assert mask == _abi.VFAM_INTENSITY and req == ["3MEAN"] + f3.NGTDM_3D + ["3GLSZM_ZP"] + f3.GLRLM_3D
    assert f3.zone_mask(req) == 3 and f3.tex_mask(req) == _abi.VTEX_NGTDM
    assert f3.expand3d_zones(["*3D_GLSZM*"]) == (0, f3.GLSZM_3D) and f3.zone_mask(f3.GLSZM_3D) == 2 and f3.zone_mask(f3.GLCM_3D) == 0
    assert f3.expand3d_zones(["*3D_GLCM*", "*3D_GLDM*"]) == f3.expand3d(["*3D_GLCM*", "*3D_GLDM*"])
    assert f3.table_column("3GLRLM_SRE") == "3GLRLM_SRE_0" and f3.table_column("3GLRLM_SRE_AVE") == "3GLRLM_SRE_AVE" and f3.table_column("3GLSZM_SAE") == "3GLSZM_SAE"
    for bad in (["*3D_GLDZM*"], ["*3D_ALL*"], ["3GLDZM_SDE"], ["MEAN"], []):
        with pytest.raises(ValueError):
            f3.expand3d_zones(bad)
    n = nyxus_amd.Nyxus3DZones(["*3D_GLRLM*", "*3D_GLSZM*", "*3D_GLCM*"], coarse_gray_depth=32)
    cols, sel = n._columns()
    assert cols == f3.GLCM_3D + f3.GLSZM_3D + f3.GLRLM_3D
    names = _lib.vol_column_names(_abi.VFAM_GLCM, n._settings) + _lib.volzone_column_names(3)
    assert [names[i] for i in sel] == [f3.table_column(c) for c in cols]
    assert isinstance(n, nyxus_amd.Nyxus3D)
    for call in (n.featurize_directory, n.featurize_files):
        with pytest.raises(NotImplementedError):
            call("a", "b")
    with pytest.raises(ValueError, match="Neighbor distance"):
        nyxus_amd.Nyxus3DZones(["*3D_GLSZM*"], neighbor_distance=0)


def test_expand3d_and_nyxus3d_still_refuse():
    for f in ("*3D_GLRLM*", "*3D_GLSZM*", "3GLRLM_SRE", "3GLSZM_SAE", "3GLRLM_SRE_AVE"):
        with pytest.raises(ValueError, match="3D_ALL_INTENSITY.*3D_GLCM"):
            featureset3d.expand3d([f])
        with pytest.raises(ValueError):
            nyxus_amd.Nyxus3D([f])
    n = nyxus_amd.Nyxus3D(["*3D_GLDM*"])
    for key in ("3glrlm/greydepth=5", "3glszm/greydepth=5"):
        with pytest.raises(ValueError, match="3gldm/greydepth.*3ngtdm/greydepth.*3ngtdm/radius"):
            n.set_metaparam(key)
    assert not hasattr(n, "_zone_mask")


def test_metaparameters():
    n = nyxus_amd.Nyxus3DZones(["*3D_GLRLM*", "*3D_GLSZM*", "*3D_GLDM*"])
    for key in ("3glrlm/greydepth", "3glszm/greydepth", "3glsz/greydepth", "3gldm/greydepth", "3ngtdm/greydepth", "3ngtdm/radius"):
        assert n.get_metaparam(key) == 0.0                 # the reference's defaults
    n.set_metaparam("3glrlm/greydepth=-24")
    n.set_metaparam(" 3glszm/greydepth = 12 ")
    n.set_metaparam("3gldm/greydepth=64")
    n.set_metaparam("3ngtdm/radius=2")
    assert (n.get_metaparam("3glrlm/greydepth"), n.get_metaparam("3glszm/greydepth"), n.get_metaparam("3glsz/greydepth")) == (-24.0, 12.0, 12.0)
    assert (n.get_metaparam("3gldm/greydepth"), n.get_metaparam("3ngtdm/radius")) == (64.0, 2.0)
    assert (n._zone_settings.glrlm_grey_depth, n._zone_settings.glszm_grey_depth, n._tex_settings.gldm_grey_depth) == (-24, 12, 64)
    for bad, pat in (("3glrlm/greydepth=abc", 'cannot parse value "abc" of 3glrlm/greydepth: expecting an integer'),
                     ("3glszm/greydepth=1.5", 'cannot parse value "1.5" of 3glszm/greydepth: expecting an integer'),
                     ("3glszm/greydepth=99999999999", "expecting an integer"), ("3glrlm/greydepth", "expecting <feature>/<parameter>=<value>"),
                     ("3glsz/greydepth=4", "Invalid metaparameter name"), ("3gldzm/greydepth=4", "Invalid metaparameter name"),
                     ("3ngtdm/radius=0", "expecting a positive integer")):
        with pytest.raises(ValueError, match=pat):
            n.set_metaparam(bad)
    with pytest.raises(ValueError, match="Invalid metaparameter name"):
        n.get_metaparam("3gldzm/greydepth")
    assert n.get_metaparam("3glrlm/greydepth") == -24.0     # a refused value changes nothing


def test_the_api_fixture_names_the_requested_columns():
    api = json.load(open(os.path.join(HERE, "golden", "volzone", "api_expected.json")))
    _, req = featureset3d.expand3d_zones(api["features"])
    assert api["columns"] == req == featureset3d.GLSZM_3D + featureset3d.GLRLM_3D
    assert np.array(api["numeric"]).shape == (len(api["labels"]), 48)


def _moved(a, b, names):
    rel = volzone_cases.rel_diff(a, b, names)
    return float(rel.max())


def test_one_count_moves_a_column_by_more_than_ten_times_the_tolerance():
    """What the GPU tolerance can see: one count moved to the neighbouring cell of any matrix (a run or a zone one cell longer or shorter)
    moves some column of its block by more than 10 x SEAM_TOL, on every edge case and on the large recorded ROIs."""
    names = volzone_cases.column_names()
    extra = [("rule", volzone_cases.batch("rule"), *volzone_cases.settings("none")), ("snakes", volzone_cases.batch("snakes"), *volzone_cases.settings("none"))]
    least = np.inf
    for name, b, s, t in volzone_edge_cases.cases() + extra:
        for r in range(b.n_roi):
            T = volzone_ref.tables(b, r, s, t)
            base = volzone_ref.columns(T, s, t)
            for which in list(range(13)) + ["zones"]:
                for up in (True, False):
                    U = volzone_ref.move_count(T, which, up)
                    if U is None:
                        continue
                    got = volzone_ref.columns(U, s, t)
                    cols = slice(224, 240) if which == "zones" else [c * 13 + which for c in range(16)]
                    d = _moved(got[None, cols], base[None, cols], [names[i] for i in (range(224, 240) if which == "zones" else cols)])
                    least = min(least, d)
                    assert d > 10 * SEAM_TOL, (name, r, which, up, d)
    print(f"smallest largest-column move for one count: {least:.3e}")
