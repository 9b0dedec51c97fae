"""The volume distance-zone class without a GPU: tests/voldzone_ref.py against the values recorded from the reference's own class
(tests/golden/voldzone), the structure of the cases (seam crossings, diagonal arms, the distance quirks, Nd at the lane seam, the metrics
on both sides of the LDS bound), the rule that takes ROIs out of the comparison, expansion, column order and refusals of the new and the
old Python classes, and what the GPU tolerance can see: one moved count."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, featureset3d
from tests import voldzone_cases, voldzone_edge_cases, voldzone_ref, volzone_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "voldzone", "voldzone_reference.npz"))
GPU_TOL = 1e-10              # TOL of tests/test_voldzone_gpu.py


@pytest.mark.parametrize("bname,mode", voldzone_cases.CASES)
def test_restatement_matches_the_recordings(bname, mode):
    b = voldzone_cases.batch(bname)
    s = voldzone_cases.settings(mode)
    assert not voldzone_cases.rule_excluded(b, s).any()    # the reference was never run where it is undefined
    want = GOLD[voldzone_cases.case_name(bname, mode)]
    got = voldzone_ref.table(b, s)
    assert (np.isnan(got) == np.isnan(want)).all() and (np.isinf(got) == np.isinf(want)).all()
    bad, rel = voldzone_cases.compare(got, want)
    assert not bad, bad[:10]
    assert rel < 1e-12                                     # the formulas in the reference's operation order: rounding of the sums only


@pytest.mark.parametrize("bname,mode", voldzone_cases.RULE_CASES)
def test_the_rule_batch_is_recorded_from_the_restatement(bname, mode):
    b = voldzone_cases.batch(bname)
    s = voldzone_cases.settings(mode)
    ex = voldzone_cases.rule_excluded(b, s)
    flat = b.max_inten == b.min_inten
    assert (ex == ~flat).all() and ex.sum() == 4
    assert voldzone_cases.case_name(bname, mode) not in GOLD
    got = voldzone_ref.table(b, s)
    assert (voldzone_cases.rel_diff(got, GOLD[voldzone_cases.case_name(bname, mode) + "__restated"]) <= 1e-13).all()
    assert (got[flat] == s.soft_nan).all() and np.isfinite(got[ex]).all()
    # the rule reads inputs and settings alone: IBSI mode and the other binnings exclude nothing but an ROI without voxels
    for m in ("ibsi", "matlab", "none"):
        assert not voldzone_cases.rule_excluded(b, voldzone_cases.settings(m)).any()
    e = voldzone_cases.with_empty(voldzone_cases.batch("full"), at=2)
    assert voldzone_cases.rule_excluded(e, voldzone_cases.settings("matlab")).tolist() == [False, False, True] + [False] * (e.n_roi - 3)
    assert voldzone_cases.rule_excluded(e, voldzone_cases.settings("radiomics")).sum() == 1          # full boxes without a zero voxel


def test_distance_map_is_the_reference_walk():
    rng = np.random.default_rng(5)
    for _ in range(40):
        d, h, w = (int(v) for v in rng.integers(1, 8, 3))
        D = rng.integers(0, 3, (d, h, w))
        M = voldzone_ref.dist_map(D)
        want = np.array([[[voldzone_ref.dist2border_walk(D, x, y, z) for x in range(w)] for y in range(h)] for z in range(d)])
        assert (M == want).all()
        assert M.max() <= min(w, h) // 2 + 2               # the pitch of the kernel's table (roi_voldzone.h)


def test_distance_quirks():
    b = voldzone_cases.batch("conn")
    s = voldzone_cases.settings("ibsi")
    # a hole at x == 1, y == 3 of a 7 x 7 plane
    T = voldzone_ref.tables(b, voldzone_cases.CONN["hole_near_face"], s)
    M = T["dist"][0]
    assert M[3, 0] == 1                                    # on the face: 1
    assert M[3, 2] == 2                                    # directly beside a level-0 cell: 2
    assert M[2, 1] == 2 and M[4, 1] == 2                   # x == 1: 2 (the face cell x0 == 0 counts as the border)
    assert M[3, 3] == 3                                    # two cells from the hole; 4 from the faces
    assert (M[:, 0] == 1).all() and (M[:, 6] == 1).all() and (M[0, :] == 1).all() and (M[6, :] == 1).all()
    assert M[2, 2] == 3 and M[3, 4] == 3                   # (x 4, y 3): 4 from the hole, 3 from the right face
    # a hole (a cell outside the cloud) at the centre of plane 0, a zero voxel at the centre of plane 1: both are borders
    T = voldzone_ref.tables(b, voldzone_cases.CONN["hole_centre"], s)
    assert (T["dist"][0] == T["dist"][1]).all()
    assert T["dist"][0][3, 2] == 2 and T["dist"][0][2, 3] == 2 and T["dist"][0][2, 2] == 3
    # a 9 x 9 x 3 full box: distances ignore z, every plane has the map min(x + 1, 9 - x, y + 1, 9 - y)
    T = voldzone_ref.tables(b, voldzone_cases.CONN["slab"], s)
    y, x = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    for z in range(3):
        assert (T["dist"][z] == np.minimum(np.minimum(x + 1, 9 - x), np.minimum(y + 1, 9 - y))).all()
    assert T["dist"].max() == 5 and T["matrix"].shape[1] == T["zones"][:, 1].max() <= 5            # Nd is the largest ZONE metric


def test_diagonal_arms_are_two_zones():
    b = voldzone_cases.batch("conn")
    s = voldzone_cases.settings("ibsi")
    r = voldzone_cases.CONN["arms"]
    Z = voldzone_ref.tables(b, r, s)["zones"]
    assert (Z[:, 0] == 8).sum() == 2 and sorted(Z[Z[:, 0] == 8][:, 2].tolist()) == [6, 6]         # 6-connected: two zones of 2 x 3 cells
    D = voldzone_ref.binned(b, r, s)
    lv, size = volzone_ref.components(D, 0)                # the GLSZM restatement, 26-connected: one zone
    assert (lv == 8).sum() == 1 and int(size[lv == 8][0]) == 12


def test_matlab_background_forms_level_1_zones_and_zp_counts_them():
    b = voldzone_cases.batch("conn")
    s = voldzone_cases.settings("mat4")
    r = voldzone_cases.CONN["blob"]
    D = voldzone_ref.binned(b, r, s)
    T = voldzone_ref.tables(b, r, s)
    assert D.min() == 1 and T["n"] < D.size                # no level-0 cell in the box, and cells outside the cloud
    assert D[0, 0, 0] == 1 and D[-1, -1, -1] == 1          # the corners of the box lie outside the blob: level 1
    # only the box faces are borders
    z, y, x = np.meshgrid(*[np.arange(n) for n in D.shape], indexing="ij")
    assert (T["dist"] == np.minimum(np.minimum(x + 1, D.shape[2] - x), np.minimum(y + 1, D.shape[1] - y))).all()
    Z = T["zones"]
    first = Z[0]
    assert first[0] == 1 and first[1] == 1                 # the raster-first zone starts at the corner: background, metric 1
    zp = voldzone_ref.columns(T, s)[voldzone_cases.NAMES.index("ZP")]
    assert zp == len(Z) / T["n"]                           # every zone counts, the background's too
    outside = D.size - T["n"]
    inside_only = voldzone_ref.zones6(np.where(_cloud(b, r), D, 0), T["dist"])
    assert len(Z) != len(inside_only) and outside > 0


def _cloud(b, r):
    o0, o1 = int(b.px_offset[r]), int(b.px_offset[r + 1])
    K = np.zeros((int(b.bbox_d[r]), int(b.bbox_h[r]), int(b.bbox_w[r])), bool)
    K[b.z[o0:o1], b.y[o0:o1], b.x[o0:o1]] = True
    return K


def test_edge_cases_sit_at_the_seams():
    C = {c[0]: c for c in voldzone_edge_cases.cases()}
    W = voldzone_edge_cases.CELLS_PER_WG
    _, b, s = C["wg"]
    assert [int(b.bbox_w[r]) * int(b.bbox_h[r]) * int(b.bbox_d[r]) for r in range(4)] == [W - 1, W, W + 1, 2 * W + 2]
    S = voldzone_edge_cases.seams()
    assert len(S) == 7 and sorted({ax for _, _, _, ax in S}) == ["x", "y", "z"]
    for r, c, q, ax in S:                                  # a zone of two cells whose cells lie in two cell ranges
        Z = voldzone_ref.tables(b, r, s)["zones"]
        z99 = Z[Z[:, 0] == voldzone_edge_cases.SEAM_LEVEL]
        assert len(z99) == 1 and z99[0, 2] == 2
        assert c % W == 0 and q // W < c // W              # (the -z neighbour of the third range lies in the first)
        w, h = int(b.bbox_w[r]), int(b.bbox_h[r])
        assert c - q == {"x": 1, "y": w, "z": w * h}[ax]
    _, b, s = C["lanes"]
    L = voldzone_cases.LANES
    assert [voldzone_ref.tables(b, r, s)["matrix"].shape[1] for r in range(3)] == [L - 1, L, L + 1]          # Nd
    for r in range(3):
        Z = voldzone_ref.tables(b, r, s)["zones"]
        assert sorted(Z[:, 1].tolist()) == [1, L - 1 + r] and Z[Z[:, 1] > 1][0, 2] == 1                     # the single voxel at the centre
    _, b, s = C["emit"]
    metrics = set(voldzone_ref.tables(b, 0, s)["zones"][:, 1].tolist())
    assert {voldzone_cases.SHORT_DIST - 1, voldzone_cases.SHORT_DIST, voldzone_cases.SHORT_DIST + 1} <= metrics
    _, b, s = C["degenerate"]
    got = voldzone_ref.table(b, s)
    flat = (b.counts() == 0) | (b.max_inten == b.min_inten)
    assert s.soft_nan == -7.5 and flat.tolist() == [True, True, True, True, False]
    assert (got[flat] == -7.5).all() and np.isfinite(got[~flat]).all()


def test_expansion_and_column_order():
    f3 = featureset3d
    assert len(f3.GLDZM_3D) == 18 and f3.GLDZM_3D[0] == "3GLDZM_SDE" and f3.GLDZM_3D[-1] == "3GLDZM_ZDE"
    assert [c[len("3GLDZM_"):] for c in f3.GLDZM_3D] == voldzone_cases.NAMES
    assert set(f3.GROUPS_3D_DZONES) == {"*3D_GLDZM*"}
    # Feature3D order (featureset.h): intensity, GLCM, GLDM, GLDZM, NGLDM, NGTDM, GLSZM, GLRLM
    assert f3.ORDER_3D_DZONES == f3.INTENSITY_3D + f3.GLCM_3D + f3.GLDM_3D + f3.GLDZM_3D + f3.NGLDM_3D + f3.NGTDM_3D + f3.GLSZM_3D + f3.GLRLM_3D
    assert [c for c in f3.ORDER_3D_DZONES if c not in f3.GLDZM_3D] == f3.ORDER_3D_ZONES
    mask, req = f3.expand3d_dzones(["*3d_gldzm*", "3GLSZM_ZP", "*3D_NGLDM*", "*3D_GLDM*", "3mean"])
    assert mask == _abi.VFAM_INTENSITY and req == ["3MEAN"] + f3.GLDM_3D + f3.GLDZM_3D + f3.NGLDM_3D + ["3GLSZM_ZP"]
    assert f3.dzone_mask(req) == _abi.VDZ_GLDZM == 1 and f3.zone_mask(req) == _abi.VZONE_GLSZM and f3.tex_mask(req) == _abi.VTEX_GLDM | _abi.VTEX_NGLDM
    assert f3.expand3d_dzones(["3gldzm_zp", "3GLDZM_SDE"]) == (0, ["3GLDZM_SDE", "3GLDZM_ZP"]) and f3.dzone_mask(f3.GLSZM_3D) == 0
    assert f3.expand3d_dzones(["*3D_GLCM*", "*3D_GLRLM*"]) == f3.expand3d_zones(["*3D_GLCM*", "*3D_GLRLM*"])
    assert f3.table_column("3GLDZM_SDE") == "3GLDZM_SDE"
    for bad in (["*3D_ALL*"], ["3GLDZM_GLE"], ["*ALL_GLDZM*"], ["GLDZM_SDE"], ["MEAN"], []):
        with pytest.raises(ValueError):
            f3.expand3d_dzones(bad)
    n = nyxus_amd.Nyxus3DDistanceZones(["*3D_GLDZM*", "*3D_GLSZM*", "*3D_GLDM*"], coarse_gray_depth=32)
    assert isinstance(n, nyxus_amd.Nyxus3DZones) and isinstance(n, nyxus_amd.Nyxus3D)
    assert n._requested == f3.GLDM_3D + f3.GLDZM_3D + f3.GLSZM_3D
    assert (n._mask, n._tex_mask, n._zone_mask, n._dzone_mask) == (0, _abi.VTEX_GLDM, _abi.VZONE_GLSZM, _abi.VDZ_GLDZM)
    assert n._settings.grey_depth == 32
    for call in (n.featurize_directory, n.featurize_files):
        with pytest.raises(NotImplementedError, match="Nyxus3DDistanceZones"):
            call("a", "b")
    with pytest.raises(ValueError, match="Neighbor distance"):
        nyxus_amd.Nyxus3DDistanceZones(["*3D_GLDZM*"], neighbor_distance=0)
    with pytest.raises(ValueError):
        nyxus_amd.Nyxus3DDistanceZones(["*3D_ALL*"])
    # the reference has no 3gldzm/greydepth metaparameter: refused, as Nyxus3DZones refuses it; the others are served as before
    with pytest.raises(ValueError, match="Invalid metaparameter name"):
        n.set_metaparam("3gldzm/greydepth=4")
    with pytest.raises(ValueError, match="Invalid metaparameter name"):
        n.get_metaparam("3gldzm/greydepth")
    n.set_metaparam("3glszm/greydepth=12")
    assert n.get_metaparam("3glszm/greydepth") == 12.0


def test_the_other_expansions_and_classes_still_refuse():
    for f in ("*3D_GLDZM*", "3GLDZM_SDE", "3gldzm_zde"):
        with pytest.raises(ValueError, match="3D_ALL_INTENSITY.*3D_GLCM"):
            featureset3d.expand3d([f])
        with pytest.raises(ValueError, match="3D_ALL_INTENSITY.*3D_GLCM"):
            featureset3d.expand3d_zones([f])
        with pytest.raises(ValueError):
            nyxus_amd.Nyxus3D([f])
        with pytest.raises(ValueError):
            nyxus_amd.Nyxus3DZones([f, "*3D_GLSZM*"])
    for cls in (nyxus_amd.Nyxus3D, nyxus_amd.Nyxus3DZones, nyxus_amd.Nyxus3DDistanceZones):
        with pytest.raises(ValueError):
            cls(["*3D_ALL*"])
    assert not hasattr(nyxus_amd.Nyxus3DZones(["*3D_GLSZM*"]), "_dzone_mask")
    assert "GLDZM" not in "".join(featureset3d.ORDER_3D_ZONES)


def test_the_api_fixture_names_the_requested_columns():
    api = json.load(open(os.path.join(HERE, "golden", "voldzone", "api_expected.json")))
    _, req = featureset3d.expand3d_dzones(api["features"])
    assert api["columns"] == req == featureset3d.GLDZM_3D
    assert np.array(api["numeric"]).shape == (len(api["labels"]), 18)


def test_one_count_moves_a_column_by_more_than_ten_times_the_tolerance():
    """What the GPU tolerance can see: one count moved to the neighbouring cell of the matrix (a zone whose metric is one larger or smaller)
    moves some column by more than 10 x the GPU tolerance, on every edge case and on the recorded connectivity cases."""
    names = voldzone_cases.column_names()
    extra = [("conn", voldzone_cases.batch("conn"), voldzone_cases.settings("ibsi")), ("rule", voldzone_cases.batch("rule"), voldzone_cases.settings("radiomics"))]
    least, moved = np.inf, 0
    for name, b, s in voldzone_edge_cases.cases() + extra:
        for r in range(b.n_roi):
            T = voldzone_ref.tables(b, r, s)
            if T is None or T["flat"]:
                continue
            base = voldzone_ref.columns(T, s)
            for up in (True, False):
                U = voldzone_ref.move_count(T, up)
                if U is None:
                    continue
                got = voldzone_ref.columns(U, s)
                d = float(voldzone_cases.rel_diff(got[None], base[None], names).max())
                least = min(least, d)
                moved += 1
                assert d > 10 * GPU_TOL, (name, r, up, d)
    assert moved > 40
    print(f"smallest largest-column move for one count: {least:.3e}")
