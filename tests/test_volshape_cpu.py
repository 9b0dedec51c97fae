"""The volume shape entry without a GPU: tests/volshape_ref.py against the values recorded from the reference's own class
(tests/golden/volshape), its two exact hulls against each other and against scipy.spatial.ConvexHull, the rank-deficient clouds, the
column catalogue and the mask refusals of the C entry, and the expansion and column order of `Nyxus3DShape`."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset3d
from tests import volshape_cases, volshape_edge_cases, volshape_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "volshape", "volshape_reference.npz"))
R = volshape_ref


@pytest.mark.parametrize("name", volshape_cases.CASES)
def test_restatement_matches_the_recordings(name):
    b = volshape_cases.batch(name)
    T, W = GOLD[name], R.table(b, volshape_cases.settings())
    fig = volshape_cases.figures(W, T, volshape_cases.eigen_compared(b))
    print(f"{name}: hull {fig['hull']:.3e}, closed forms {fig['closed']:.3e}, eigen squares {fig['lens']:.3e}, squared ratios {fig['ratios']:.3e}")
    assert (W[:, R.COL["3AREA"]] == T[:, R.COL["3AREA"]]).all()
    assert fig["hull"] <= volshape_cases.HULL_AGREE and fig["closed"] <= volshape_cases.TOL_RESTATED
    assert fig["lens"] <= volshape_cases.TOL and fig["ratios"] <= volshape_cases.TOL
    # what is not compared with the reference is pinned to the restatement's 0
    assert (W[~volshape_cases.eigen_compared(b)] == 0).all()
    assert (W[:, R.HULL[0]] == W[:, R.HULL[1]]).all() and (T[:, R.HULL[0]] == T[:, R.HULL[1]]).all()


def test_rank_deficient_clouds_are_decided_from_the_inputs():
    b = _abi.batch3d_from_rois(volshape_edge_cases.degenerate())       # a voxel, a pair, a line, a plate, a diagonal needle, an oblique plane
    assert list(volshape_cases.ranks(b)) == [0, 1, 1, 2, 1, 2]
    W = R.table(b, volshape_cases.settings())
    ok = volshape_cases.eigen_compared(b)
    assert (~ok).sum(axis=1).tolist() == [5, 4, 4, 2, 4, 2] and (W[~ok] == 0).all()
    assert (W[:, R.HULL] == 0).all()                                   # none spans three dimensions
    assert (W[1:, R.COL["3MAJOR_AXIS_LEN"]] > 0).all() and (W[[3, 5], R.COL["3MINOR_AXIS_LEN"]] > 0).all()
    # the needle's covariance has three equal rows: its two zero eigenvalues are rounding in fp64 and exact 0 here
    x, y, z, _ = R.roi_arrays(b, 4)
    assert np.linalg.matrix_rank(R.covariance(x, y, z)) == 1 and (R.eigenvalues(x, y, z)[1:] == 0).all()
    # a solid cloud keeps its three eigenvalues; a cube has them equal
    cube = _abi.batch3d_from_rois([volshape_edge_cases.full(3, 3, 3)])
    L = R.eigenvalues(*R.roi_arrays(cube, 0)[:3])
    assert volshape_cases.eigen_compared(cube).all() and np.allclose(L, L[0], rtol=1e-14) and L[0] > 0


def test_exact_hull_against_scipy_and_the_enumeration():
    from scipy.spatial import ConvexHull
    rng = np.random.default_rng(99)
    n_solid = 0
    for trial in range(80):
        d, h, w = rng.integers(1, 8, 3)
        m = rng.random((d, h, w)) < rng.choice([0.2, 0.5, 0.9])
        z, y, x = np.nonzero(m)
        if len(x) == 0:
            continue
        inten = (rng.random(len(x)) < 0.8).astype(np.uint32)
        P = np.stack([x, y, z], axis=1)[inten != 0]
        cand = R.candidates(x, y, z, inten)
        six = R.hull6v(cand) if len(cand) else 0
        assert six == (R.hull6v(P) if len(P) else 0)                   # the row extremes' plane hulls hold every hull vertex
        if 0 < len(cand) <= 16:
            assert six == R.hull6v_brute(cand)
        if len(P) and R.rank(P) == 3:
            n_solid += 1
            assert abs(ConvexHull(P).volume * 6 - six) < 1e-9 * six
        else:
            assert six == 0
    assert n_solid > 40
    for r, six in ((3, 544), (5, 2704)):                               # the lattice balls of DESIGN.md 4.5n: 90.67 and 450.67
        z, y, x = np.nonzero(volshape_edge_cases.ball_mask(r))
        assert R.hull6v(R.candidates(x, y, z, np.ones(len(x)))) == six == round(ConvexHull(np.stack([x, y, z], axis=1)).volume * 6)


def test_the_reference_hulls_contours_that_hold_every_hull_vertex():
    """build_contour_imp restated: on the recorded clouds and on the inexact ones alike the traced borders hold every vertex of the hull,
    so where the reference's volume is off, its float quickhull is what is off, not the points it is handed."""
    for name in volshape_cases.CASES + volshape_cases.INEXACT:
        b = volshape_cases.batch(name)
        for r in range(b.n_roi):
            x, y, z, v = R.roi_arrays(b, r)
            K = R.contour_points(x, y, z, v)
            lit = np.stack([x, y, z], axis=1)[v != 0]
            assert {tuple(p) for p in K.tolist()} <= {tuple(p) for p in lit.tolist()}
            assert R.hull6v(K) == R.hull6v(R.candidates(x, y, z, v)), (name, r)
    # a full plane of 4 x 3: the border is its ten outer voxels, in raster order
    g = np.arange(12)
    K = R.contour_points(g % 4, g // 4, np.zeros(12, int), np.ones(12, int))
    assert K[:, :2].tolist() == [[xx, yy] for yy in range(3) for xx in range(4) if not (yy == 1 and xx in (1, 2))]


def test_the_inexact_clouds_are_recorded_side_by_side():
    for name in volshape_cases.INEXACT:
        ref, exact = GOLD[name + "__reference_inexact"][0]
        assert exact == R.hull6_of(volshape_cases.batch(name))[0] / 6.0
        assert abs(ref - exact) / exact > 1e3 * volshape_cases.HULL_AGREE      # documents the ruling; nothing is compared with `ref`


def test_faces_and_volume_count_every_voxel():
    roi = volshape_edge_cases.dark_corners()
    x, y, z, v = (np.asarray(roi[k]) for k in ("x", "y", "z", "inten"))
    row = R.row(x, y, z, v)
    assert row[R.COL["3AREA"]] == 2 * (5 * 4 + 4 * 6 + 5 * 6) and abs(row[R.COL["3VOXEL_VOLUME"]] - 120 * (np.pi / 6) / 0.5236) < 1e-9
    assert row[R.HULL[0]] * 6 == R.hull6v(np.stack([x, y, z], axis=1)[v != 0]) < 6 * 4 * 3 * 5    # the dark corners are cut off the hull
    assert R.exposed_faces([0, 1, 3], [0, 0, 0], [0, 0, 0]) == 16


def test_catalogue_and_mask_refusals_of_the_entry():
    lib = _lib.load()
    assert lib.nyxhip_vshape_n_columns(_abi.VSHAPE_MORPHOLOGY) == 14 == _abi.VOLSHAPE_COLS
    assert _lib.volshape_column_names() == R.NAMES == featureset3d.SHAPE_3D
    import ctypes as C
    buf = C.create_string_buffer(64)
    for mask in (0, 2, 3, 1 << 31):
        assert lib.nyxhip_vshape_n_columns(mask) == -1
        assert lib.nyxhip_vshape_column_name(mask, 0, buf, 64) == 1
        with pytest.raises(_lib.NyxHipError):
            _lib.volshape_column_names(mask)
    assert lib.nyxhip_vshape_column_name(1, 14, buf, 64) == 1 and lib.nyxhip_vshape_column_name(1, -1, buf, 64) == 1
    assert lib.nyxhip_vshape_column_name(1, 13, buf, 64) == 0 and buf.value == b"3FLATNESS"
    assert lib.nyxhip_featurize_volumes_shape(None, None, 1, None, None, 14) == 1


def test_expansion_and_column_order():
    f3 = featureset3d
    assert len(f3.SHAPE_3D) == 14 and f3.SHAPE_3D[0] == "3AREA" and f3.SHAPE_3D[-1] == "3FLATNESS"
    assert set(f3.GROUPS_3D_SHAPE) == {"*3D_ALL_MORPHOLOGY*", "*3D_ALL*"}
    # Feature3D order (featureset.h): intensity, shape, GLCM, GLDM, GLDZM, NGLDM, NGTDM, GLSZM, GLRLM
    assert f3.ORDER_3D_SHAPE == f3.INTENSITY_3D + f3.SHAPE_3D + f3.GLCM_3D + f3.GLDM_3D + f3.GLDZM_3D + f3.NGLDM_3D + f3.NGTDM_3D + f3.GLSZM_3D + f3.GLRLM_3D
    assert [c for c in f3.ORDER_3D_SHAPE if c not in f3.SHAPE_3D] == f3.ORDER_3D_DZONES
    mask, req = f3.expand3d_shape(["*3d_all*"])
    assert req == f3.ORDER_3D_SHAPE and len(req) == 36 + 14 + 59 + 14 + 18 + 19 + 5 + 16 + 32 and mask == _abi.VFAM_ALL
    assert (f3.shape_mask(req), f3.dzone_mask(req), f3.zone_mask(req), f3.tex_mask(req)) == (1, 1, _abi.VZONE_ALL, _abi.VTEX_GLDM | _abi.VTEX_NGLDM | _abi.VTEX_NGTDM)
    assert f3.expand3d_shape(["*3D_ALL_MORPHOLOGY*"]) == (0, f3.SHAPE_3D)
    assert f3.expand3d_shape(["3flatness", "3GLCM_ASM", "3AREA", "3mean"]) == (_abi.VFAM_ALL, ["3MEAN", "3AREA", "3FLATNESS", "3GLCM_ASM"])
    assert f3.expand3d_shape(["*3D_GLCM*", "*3D_GLDZM*"]) == f3.expand3d_dzones(["*3D_GLCM*", "*3D_GLDZM*"]) and f3.shape_mask(f3.GLCM_3D) == 0
    for bad in (["*3D_ALL_NEIGHBOR*"], ["*3D_ALL_TEXTURE*"], ["3DIAMETER_EQUAL_VOLUME"], ["AREA"], ["*ALL_MORPHOLOGY*"], []):
        with pytest.raises(ValueError):
            f3.expand3d_shape(bad)
    n = nyxus_amd.Nyxus3DShape(["*3D_ALL_MORPHOLOGY*", "*3D_GLDZM*", "3MEAN"], coarse_gray_depth=32)
    assert isinstance(n, nyxus_amd.Nyxus3DDistanceZones)
    assert n._requested == ["3MEAN"] + f3.SHAPE_3D + f3.GLDZM_3D
    assert (n._mask, n._tex_mask, n._zone_mask, n._dzone_mask, n._shape_mask) == (_abi.VFAM_INTENSITY, 0, 0, 1, 1)
    a = nyxus_amd.Nyxus3DShape(["*3D_ALL*"])
    assert a._requested == f3.ORDER_3D_SHAPE and a._shape_mask == 1
    for call in (n.featurize_directory, n.featurize_files):
        with pytest.raises(NotImplementedError, match="Nyxus3DShape"):
            call("a", "b")
    n.set_metaparam("3glszm/greydepth=12")                             # the metaparameters of the older classes are served as before
    assert n.get_metaparam("3glszm/greydepth") == 12.0
    with pytest.raises(ValueError, match="Invalid metaparameter name"):
        n.set_metaparam("3shape/greydepth=4")


def test_the_older_expansions_and_classes_still_refuse():
    for f in ("*3D_ALL_MORPHOLOGY*", "3AREA", "3flatness", "*3D_ALL*"):
        for expand in (featureset3d.expand3d, featureset3d.expand3d_zones, featureset3d.expand3d_dzones):
            with pytest.raises(ValueError, match="3D_ALL_INTENSITY.*3D_GLCM.*the 3-D shape class"):   # their present message
                expand([f])
        for cls in (nyxus_amd.Nyxus3D, nyxus_amd.Nyxus3DZones, nyxus_amd.Nyxus3DDistanceZones):
            with pytest.raises(ValueError):
                cls([f, "*3D_GLCM*"])
    assert not hasattr(nyxus_amd.Nyxus3DDistanceZones(["*3D_GLDZM*"]), "_shape_mask")
    assert "3AREA" not in featureset3d.ORDER_3D_DZONES


def test_the_api_fixture_names_the_requested_columns():
    api = json.load(open(os.path.join(HERE, "golden", "volshape", "api_expected.json")))
    _, req = featureset3d.expand3d_shape(api["features"])
    assert api["columns"] == req == featureset3d.SHAPE_3D
    assert np.array(api["numeric"]).shape == (len(api["labels"]), 14)
    zone = json.load(open(os.path.join(HERE, "golden", "volzone", "api_expected.json")))
    assert api["metaparams"] == zone["metaparams"] and api["labels"] == zone["labels"]
