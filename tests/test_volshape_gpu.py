"""The volume shape entry on the GPU (nyxhip_featurize_volumes_shape, roi_volshape.hip) against tests/volshape_ref.py on the clouds of
tests/volshape_edge_cases.py, and `Nyxus3DShape` against the recording of tests/golden/volshape.

What is exact is held exactly: 3AREA is an integer count and the two hull columns are an integer 6 V divided by 6 (one IEEE division on
both sides), so they are compared bit for bit.  3VOXEL_VOLUME and the closed forms are held within TOL = 1e-10: the kernel multiplies where
the reference adds voxel by voxel (at most 5e4 voxels here: a relative 5e4 x 2^-53 = 6e-12 in the worst case), and pow / sqrt differ in
the last bit.  The eigen columns are held as squares -- (len / 4)^2 within 1e-10 x lambda_max, the squared ratios within 1e-10 -- because a
square root blows an absolute error up without bound near a zero eigenvalue.  A call that returns has found the device status word 0."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import vol_cases, volshape_cases, volshape_edge_cases, volshape_ref
from tests.volshape_device import device_rows

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SH = _abi.VSHAPE_MORPHOLOGY
R = volshape_ref


def same(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def held(got, want, h6, label):
    """the rules of the module's docstring; prints every figure before it asserts"""
    fig = volshape_cases.figures(got, want)
    print(f"{label}: closed forms {fig['closed']:.3e}, eigen squares {fig['lens']:.3e} of lambda_max, squared ratios {fig['ratios']:.3e}")
    assert (got[:, R.COL["3AREA"]] == want[:, R.COL["3AREA"]]).all(), (label, got[:, 0], want[:, 0])
    for c in R.HULL:
        assert same(got[:, c].copy(), np.asarray(h6, np.float64) / 6.0).all(), (label, (got[:, c] * 6).tolist(), list(h6))
    assert fig["closed"] <= volshape_cases.TOL and fig["lens"] <= volshape_cases.TOL and fig["ratios"] <= volshape_cases.TOL, (label, fig)


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own on cuda:0: the workspaces this entry grows stay out of the context the other test files share."""
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", ["degenerate", "boxes", "round", "holes", "long", "lds"])
def test_rows_against_the_restatement(ctx, name):
    b = volshape_edge_cases.groups()[name]
    want, h6 = volshape_edge_cases.reference(name)
    s = _abi.default_settings(64)
    got = ctx.volumes_shape_host(b, SH, s)
    held(got, want, h6, name)
    if name == "degenerate":
        assert (h6 == 0).all() and (got[:, R.HULL] == 0).all()
        ranks = [R.rank(np.stack(R.roi_arrays(b, r)[:3], axis=1)) for r in range(b.n_roi)]
        assert ranks == [0, 1, 1, 2, 1, 2]
        for r, k in enumerate(ranks):                      # the eigen columns beyond the rank are the restatement's 0
            assert (want[r, R.LENS[k:]] == 0).all() and (want[r, R.RATIOS[max(k - 1, 0):]] == 0).all()
    if name == "boxes":                                    # a cube: three equal eigenvalues
        assert abs(got[0, R.COL["3ELONGATION"]] - 1) < 1e-9 and abs(got[2, R.COL["3FLATNESS"]] - 1) < 1e-9
    if name == "lds":                                      # one below and one above the switch between LDS and the workspace
        n = [len(R.candidates(*R.roi_arrays(b, r))) for r in range(b.n_roi)]
        assert n == [volshape_edge_cases.LDS_CAND - 1, volshape_edge_cases.LDS_CAND + 1]
    if name in ("boxes", "holes"):
        assert same(device_rows(ctx, b, s), got).all()


def test_a_row_has_the_same_bits_however_it_is_asked_for(ctx):
    s = _abi.default_settings(64)
    G = volshape_edge_cases.groups()
    parts = [G[n] for n in ("degenerate", "boxes", "round", "holes")]
    rois = []
    for p in parts:
        rois += [p.select([r]) for r in range(p.n_roi)]
    order = list(range(len(rois)))
    cat = lambda idx: _abi.HostBatch3D(*[np.concatenate([getattr(rois[i], k) for i in idx]) if k != "px_offset" else
                                          np.concatenate([[0], np.cumsum([int(rois[i].px_offset[1]) for i in idx])]).astype(np.uint64)
                                          for k in ("roi_label", "px_offset", "x", "y", "z", "inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten")])
    mixed_b = cat(order)
    mixed = ctx.volumes_shape_host(mixed_b, SH, s)
    k = 0
    for p, n in zip(parts, ("degenerate", "boxes", "round", "holes")):   # alone | in the mixed batch
        held(mixed[k:k + p.n_roi], *volshape_edge_cases.reference(n), "mixed/" + n)
        assert same(ctx.volumes_shape_host(p, SH, s), mixed[k:k + p.n_roi]).all()
        k += p.n_roi
    for r in (0, 3, 5, 8, 12, len(rois) - 1):              # single ROIs: a launch sized by the ROI alone
        assert same(ctx.volumes_shape_host(rois[r], SH, s), mixed[r:r + 1]).all(), r
    assert same(ctx.volumes_shape_host(cat(order[::-1]), SH, s)[::-1], mixed).all()       # reversed batch order
    assert same(ctx.volumes_shape_host(mixed_b, SH, s, stated=True), mixed).all()         # stated against derived extrema
    assert same(device_rows(ctx, mixed_b, s, stated=True), mixed).all()                   # device memory, stated and derived
    assert same(device_rows(ctx, mixed_b, s, stated=False), mixed).all()
    # chunks: budgets that hold a few ROIs' workspaces, then exactly one
    with pytest.raises(_lib.NyxHipError, match=r"one ROI \((\d+) bytes\)") as ei:
        ctx.volumes_shape_host(mixed_b, SH, s, max_device_bytes=64)
    assert ei.value.code == 5
    per_roi = int(str(ei.value).split("one ROI (")[1].split(" bytes")[0])
    for budget in (3 * per_roi + 5, per_roi):
        assert same(ctx.volumes_shape_host(mixed_b, SH, s, max_device_bytes=budget), mixed).all(), budget
    assert same(device_rows(ctx, mixed_b, s, max_device_bytes=2 * per_roi), mixed).all()


def test_empty_rois_and_soft_nan(ctx):
    full = volshape_edge_cases.full
    empty = {"x": [], "y": [], "z": [], "inten": [], "box": (3, 3, 3)}
    b = _abi.batch3d_from_rois([full(2, 3, 2), empty, full(3, 2, 2), dict(empty, box=(0, 0, 0))])
    for nan in (0.0, -7.5):
        s = _abi.default_settings(64)
        s.soft_nan = nan
        got = ctx.volumes_shape_host(b, SH, s)
        assert (got[[1, 3]] == nan).all()
        want = R.table(b, s)
        held(got[[0, 2]], want[[0, 2]], R.hull6_of(b)[[0, 2]], f"beside empty ROIs, soft_nan {nan}")
        assert same(device_rows(ctx, b, s), got).all()


def test_refusals(ctx):
    b = volshape_edge_cases.groups()["boxes"]
    s = _abi.default_settings(64)
    for mask in (0, 2, 3, 1 << 12):
        with pytest.raises(_lib.NyxHipError) as ei:
            ctx.volumes_shape_host(b, mask, s)
        assert ei.value.code == 1
    import ctypes as C
    out = np.zeros((b.n_roi, 14))
    cb = b.c_struct()
    assert ctx._lib.nyxhip_featurize_volumes_shape(ctx._h, C.byref(cb), SH, C.byref(s), out.ctypes.data, 13) == 1      # ld below the columns
    assert ctx._lib.nyxhip_featurize_volumes_shape(ctx._h, C.byref(cb), SH, None, out.ctypes.data, 14) == 1
    o1, o2 = int(b.px_offset[1]), int(b.px_offset[2])
    out_ = _abi.HostBatch3D(b.roi_label[1:2], [0, o2 - o1], b.x[o1:o2], b.y[o1:o2], b.z[o1:o2], b.inten[o1:o2], [3], [4], [4], b.min_inten[1:2], b.max_inten[1:2])
    with pytest.raises(_lib.NyxHipError, match="outside its box") as ei:
        ctx.volumes_shape_host(out_, SH, s)
    assert ei.value.code == 1
    want, h6 = volshape_edge_cases.reference("boxes")      # the context serves the next call
    held(ctx.volumes_shape_host(b, SH, s), want, h6, "after the refusals")


def test_nyxus3dshape_featurize_against_the_recordings():
    gold = os.path.join(HERE, "golden")
    api = json.load(open(os.path.join(gold, "volshape", "api_expected.json")))
    I, M = vol_cases.api_volumes()
    f3 = nyxus_amd.featureset3d
    depth = api["coarse_gray_depth"]
    n = nyxus_amd.Nyxus3DShape(["*3D_ALL*"], coarse_gray_depth=depth)
    older = nyxus_amd.Nyxus3DDistanceZones(["*3D_ALL_INTENSITY*", "*3D_GLCM*", "*3D_GLDM*", "*3D_GLDZM*", "*3D_NGLDM*", "*3D_NGTDM*", "*3D_GLSZM*", "*3D_GLRLM*"],
                                           coarse_gray_depth=depth)
    for m in api["metaparams"]:
        n.set_metaparam(m)
        older.set_metaparam(m)
    df = n.featurize(I, M, intensity_names=["a.vol", "b.vol"], label_names=["a.seg", "b.seg"])
    lead = ["intensity_image", "mask_image", "ROI_label", "t_index"]
    assert list(df.columns) == lead + f3.ORDER_3D_SHAPE    # Feature3D order: the shape block directly behind the intensity block
    assert list(df.columns)[4 + 36:4 + 36 + 14] == api["columns"] == R.NAMES and df.columns[4 + 50] == "3GLCM_ACOR"
    assert list(df["ROI_label"]) == api["labels"] and list(df["intensity_image"]) == [["a.vol", "b.vol"][v] for v in api["volumes"]]
    got, want = df[api["columns"]].to_numpy(), np.array(api["numeric"])
    fig = volshape_cases.figures(got, want)
    print(f"api: closed forms {fig['closed']:.3e}, eigen squares {fig['lens']:.3e}, squared ratios {fig['ratios']:.3e}, hull {fig['hull']:.3e}")
    assert (got[:, 0] == want[:, 0]).all() and fig["hull"] <= volshape_cases.HULL_AGREE
    assert max(fig["closed"], fig["lens"], fig["ratios"]) <= volshape_cases.TOL
    # what Nyxus3DDistanceZones serves has its bits, and the fixtures of the other four entries hold for the same call
    od = older.featurize(I, M, intensity_names=["a.vol", "b.vol"], label_names=["a.seg", "b.seg"])
    rest = [c for c in f3.ORDER_3D_SHAPE if c not in f3.SHAPE_3D]
    assert list(od.columns) == lead + rest
    assert same(df[rest].to_numpy().copy(), od[rest].to_numpy().copy()).all()
    from tests import voldzone_cases, voltex_cases, volzone_cases
    load = lambda fam: json.load(open(os.path.join(gold, fam, "api_expected.json")))
    vol, tex, zone, dz = load("vol")["cases"]["groups"], load("voltex")["cases"]["set"], load("volzone"), load("voldzone")
    assert set(tex["metaparams"]) <= set(api["metaparams"]) and zone["metaparams"] == api["metaparams"] and dz["coarse_gray_depth"] == depth
    for fix, cmp in ((vol, vol_cases.compare), (tex, voltex_cases.compare), (zone, volzone_cases.compare), (dz, voldzone_cases.compare)):
        bad = cmp(df[fix["columns"]].to_numpy(), np.array(fix["numeric"]), fix["columns"])[0]
        assert not bad, bad[:10]
    only = nyxus_amd.Nyxus3DShape(["3FLATNESS", "3area", "*3D_ALL_MORPHOLOGY*"]).featurize(I, M)
    assert list(only.columns) == lead + R.NAMES
    assert same(only[R.NAMES].to_numpy().copy(), df[R.NAMES].to_numpy().copy()).all()
