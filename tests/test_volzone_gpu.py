"""The volume zone entry on the GPU (nyxhip_featurize_volumes_zones, roi_volzone.hip): the 224 GLRLM and 16 GLSZM columns against the
values recorded from the reference's own classes (tests/golden/volzone) under the project's policy (volzone_cases.compare:
parity.REL_TOL), the edge and seam cases against tests/volzone_ref.py within SEAM_TOL, the level cap, the refusals, and the bits of a row
across batch order, memory kind, stated against derived extrema, chunks, classes and binned boxes.

SEAM_TOL.  The integer matrices agree exactly; what differs between the kernels' closing and the restatement is the order of the fp64
sums (a lane sums its run lengths or list entries and the lanes are added in lane order; NumPy sums pairwise).  The largest relative
differences printed on an MI355X are in DESIGN.md 4.5l; SEAM_TOL lies more than 100 x above them, and tests/test_volzone_cpu.py shows that
one moved count moves a column by more than 10 x SEAM_TOL.  The variance columns (GLV, RV, ZV) are sums of p (x - mu)^2: where all the
mass sits on one x the exact value is 0 and either side may land on rounding noise of mu, so for them the difference is measured against
max(|value|, 1) (volzone_cases.floor), as test_voltex_gpu.FLOOR does."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import volzone_cases, volzone_edge_cases, volzone_ref
from tests.volzone_device import device_rows

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "volzone", "volzone_reference.npz"))
SEAM_TOL = 1e-10
R = volzone_cases.N_GLRLM
ALL = _abi.VZONE_ALL


def same(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own on cuda:0: the workspaces these entries grow stay out of the context the other test files share."""
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("bname,mode", volzone_cases.CASES)
def test_rows_match_the_reference_classes(ctx, bname, mode):
    b = volzone_cases.batch(bname)
    s, t = volzone_cases.settings(mode)
    want = GOLD[volzone_cases.case_name(bname, mode)]
    got = ctx.volumes_zones_host(b, ALL, s, t)
    bad, rel = volzone_cases.compare(got, want)
    print(f"{bname}/{mode}: largest relative difference {rel:.3e}")
    assert not bad, bad[:10]
    # the columns the rule names are this package's: held to the restatement, within the seam bound
    ex = volzone_cases.rule_excluded(b, s, t)
    if ex.any():
        rr = volzone_cases.rel_diff(got, volzone_ref.table(b, s, t))
        assert (rr[ex] <= SEAM_TOL).all()
    # each class alone has the bits it has beside the other
    assert same(ctx.volumes_zones_host(b, _abi.VZONE_GLRLM, s, t), got[:, :R]).all()
    assert same(ctx.volumes_zones_host(b, _abi.VZONE_GLSZM, s, t), got[:, R:]).all()


@pytest.mark.parametrize("case", volzone_edge_cases.cases() + [(f"{n}/{m}", volzone_cases.batch(n), *volzone_cases.settings(m)) for n, m in
                                                               (("snakes", "none"), ("conn", "mat4"), ("runs", "matlab"), ("rule", "none"))], ids=lambda c: c[0])
def test_edge_and_seam_rows_against_the_restatement(ctx, case):
    name, b, s, t = case
    want = volzone_ref.table(b, s, t)
    got = ctx.volumes_zones_host(b, ALL, s, t)
    assert (np.isnan(got) == np.isnan(want)).all() and (np.isinf(got) == np.isinf(want)).all()
    rel = volzone_cases.rel_diff(got, want)
    print(f"{name}: largest relative difference GPU vs restatement {rel.max():.3e}")
    assert (rel <= SEAM_TOL).all(), (name, np.argwhere(rel > SEAM_TOL)[:5].tolist())
    assert same(device_rows(ctx, b, s, t), got).all()


def test_level_cap_host_and_device(ctx):
    b = volzone_cases.batch("boxes")
    big = b.n_roi - 2                                                                     # the 12^3 blob
    s, t = volzone_cases.settings("cap")                                                  # exactly at the cap: served
    assert np.isfinite(ctx.volumes_zones_host(b, ALL, s, t)[big]).all()
    cap = str(volzone_cases.LEVEL_CAP)
    for field, bit in (("glrlm_grey_depth", _abi.VZONE_GLRLM), ("glszm_grey_depth", _abi.VZONE_GLSZM)):
        for v in (volzone_cases.LEVEL_CAP + 1, -(volzone_cases.LEVEL_CAP + 1)):
            s, t = volzone_cases.settings("radiomics")
            setattr(t, field, v)
            with pytest.raises(_lib.NyxHipError, match=cap + ".*" + field) as ei:
                ctx.volumes_zones_host(b, ALL, s, t)
            assert ei.value.code == 4
            assert np.isfinite(ctx.volumes_zones_host(b, ALL & ~bit, s, t)[big]).all()    # the other class does not read the setting
            s.ibsi = 1                                                                    # IBSI mode does not read it either
            assert np.isfinite(ctx.volumes_zones_host(b, ALL, s, t)[big]).all()
    # IBSI mode / grey depth 0: the largest intensity of an ROI is the level count -- found on the device, with a good ROI beside it
    def one(v):
        z, y, x = np.meshgrid(np.arange(2), np.arange(2), np.arange(3), indexing="ij")
        return {"x": x.ravel(), "y": y.ravel(), "z": z.ravel(), "inten": np.r_[np.arange(1, 12), v].astype(np.uint32), "origin": (0, 0, 0), "box": (3, 2, 2)}
    at, over = _abi.batch3d_from_rois([one(volzone_cases.LEVEL_CAP)]), _abi.batch3d_from_rois([one(5), one(volzone_cases.LEVEL_CAP + 1)])
    si, ti = volzone_cases.settings("ibsi")
    s0, t0 = volzone_cases.settings("none")
    for ss, tt in ((si, ti), (s0, t0)):
        got = ctx.volumes_zones_host(at, ALL, ss, tt)                                     # 128 levels: served, and right
        assert (volzone_cases.rel_diff(got, volzone_ref.table(at, ss, tt)) <= SEAM_TOL).all()
        for bit in (_abi.VZONE_GLRLM, _abi.VZONE_GLSZM, ALL):
            with pytest.raises(_lib.NyxHipError, match=cap) as ei:
                ctx.volumes_zones_host(over, bit, ss, tt)
            assert ei.value.code == 4
    with pytest.raises(_lib.NyxHipError) as ei:
        device_rows(ctx, over, si, ti)
    assert ei.value.code == 4
    # the context serves the next call
    s, t = volzone_cases.settings("radiomics")
    assert same(ctx.volumes_zones_host(over.select([0]), ALL, s, t), ctx.volumes_zones_host(over, ALL, s, t)[:1]).all()


def test_refusals(ctx):
    b = volzone_cases.batch("boxes")
    s, t = volzone_cases.settings("matlab")
    for mask in (0, 4, 1 << 12, ALL | 4):
        with pytest.raises(_lib.NyxHipError) as ei:
            ctx.volumes_zones_host(b, mask, s, t)
        assert ei.value.code == 1
    import ctypes as C
    out = np.zeros((b.n_roi, 240))
    cb = b.c_struct()
    assert ctx._lib.nyxhip_featurize_volumes_zones(ctx._h, C.byref(cb), ALL, C.byref(s), C.byref(t), out.ctypes.data, 239) == 1     # ld below the columns
    assert ctx._lib.nyxhip_featurize_volumes_zones(ctx._h, C.byref(cb), ALL, C.byref(s), None, out.ctypes.data, 240) == 1
    big = _abi.HostBatch3D(b.roi_label[:1], b.px_offset[:2], b.x[:1], b.y[:1], b.z[:1], b.inten[:1], [257], [256], [256], b.min_inten[:1], b.max_inten[:1])
    with pytest.raises(_lib.NyxHipError, match="256") as ei:
        ctx.volumes_zones_host(big, ALL, s, t)
    assert ei.value.code == 5
    o4, o5 = int(b.px_offset[4]), int(b.px_offset[5])
    out_ = _abi.HostBatch3D(b.roi_label[4:5], [0, 8], b.x[o4:o5], b.y[o4:o5], b.z[o4:o5], b.inten[o4:o5], [2], [2], [1], b.min_inten[4:5], b.max_inten[4:5])
    for bit in (_abi.VZONE_GLRLM, _abi.VZONE_GLSZM):
        with pytest.raises(_lib.NyxHipError, match="outside its box") as ei:
            ctx.volumes_zones_host(out_, bit, s, t)
        assert ei.value.code == 1
    with pytest.raises(_lib.NyxHipError, match="max_device_bytes") as ei:
        ctx.volumes_zones_host(volzone_cases.batch("rule"), ALL, s, t, max_device_bytes=4096)
    assert ei.value.code == 5
    assert np.isfinite(ctx.volumes_zones_host(b, ALL, s, t)[b.n_roi - 2]).all()           # the context serves the next call


def test_an_roi_without_voxels_is_soft_nan(ctx):
    b0 = volzone_cases.batch("boxes")
    b = volzone_cases.with_empty(b0, at=5)
    s, t = volzone_cases.settings("softnan")
    got = ctx.volumes_zones_host(b, ALL, s, t)
    assert (got[5] == -7.5).all()
    assert same(np.delete(got, 5, axis=0), ctx.volumes_zones_host(b0, ALL, s, t)).all()
    assert same(device_rows(ctx, b, s, t), got).all()


def test_a_row_has_the_same_bits_however_it_is_asked_for(ctx):
    s, t = volzone_cases.settings("mixed")                                                # two binned boxes
    parts = [volzone_cases.batch(n) for n in ("boxes", "conn", "snakes", "rule")] + [volzone_edge_cases.cases()[k][1] for k in (1, 3)]
    rois = []
    for p in parts:
        rois += [p.select([r]) for r in range(p.n_roi)]
    order = list(range(len(rois)))
    cat = lambda idx: _abi.HostBatch3D(*[np.concatenate([getattr(rois[i], k) for i in idx]) if k != "px_offset" else
                                          np.concatenate([[0], np.cumsum([int(rois[i].px_offset[1]) for i in idx])]).astype(np.uint64)
                                          for k in ("roi_label", "px_offset", "x", "y", "z", "inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten")])
    mixed_b = cat(order)
    mixed = ctx.volumes_zones_host(mixed_b, ALL, s, t)
    k = 0
    for p in parts:                                                                      # alone | in the mixed batch
        assert same(ctx.volumes_zones_host(p, ALL, s, t), mixed[k:k + p.n_roi]).all()
        k += p.n_roi
    for r in (0, 4, 11, 16, 20, 25, len(rois) - 13, len(rois) - 1):                       # single ROIs: a launch sized by the ROI alone
        assert same(ctx.volumes_zones_host(rois[r], ALL, s, t), mixed[r:r + 1]).all(), r
    assert same(ctx.volumes_zones_host(cat(order[::-1]), ALL, s, t)[::-1], mixed).all()  # reversed batch order
    assert same(ctx.volumes_zones_host(mixed_b, ALL, s, t, stated=True), mixed).all()     # stated against derived extrema
    assert same(device_rows(ctx, mixed_b, s, t, stated=True), mixed).all()                # device memory, stated and derived
    assert same(device_rows(ctx, mixed_b, s, t, stated=False), mixed).all()
    assert same(ctx.volumes_zones_host(mixed_b, _abi.VZONE_GLRLM, s, t), mixed[:, :R]).all()   # each class alone
    assert same(ctx.volumes_zones_host(mixed_b, _abi.VZONE_GLSZM, s, t), mixed[:, R:]).all()
    # one binned box for both classes gives each class the bits it has with a box of its own
    t1 = _abi.VolZoneSettings(t.glrlm_grey_depth, t.glrlm_grey_depth)
    t2 = _abi.VolZoneSettings(t.glszm_grey_depth, t.glszm_grey_depth)
    assert same(ctx.volumes_zones_host(mixed_b, ALL, s, t1)[:, :R], mixed[:, :R]).all()
    assert same(ctx.volumes_zones_host(mixed_b, ALL, s, t2)[:, R:], mixed[:, R:]).all()
    # chunks: budgets that hold a few ROIs' workspaces, then exactly one
    with pytest.raises(_lib.NyxHipError, match=r"one ROI \((\d+) bytes\)") as ei:
        ctx.volumes_zones_host(mixed_b, ALL, s, t, max_device_bytes=4096)
    per_roi = int(str(ei.value).split("one ROI (")[1].split(" bytes")[0])
    for budget in (3 * per_roi + 5, per_roi):
        assert same(ctx.volumes_zones_host(mixed_b, ALL, s, t, max_device_bytes=budget), mixed).all(), budget
    assert same(device_rows(ctx, mixed_b, s, t, max_device_bytes=2 * per_roi), mixed).all()


def test_nyxus3dzones_featurize_against_the_recording():
    api = json.load(open(os.path.join(HERE, "golden", "volzone", "api_expected.json")))
    I, M = volzone_cases.api_volumes()
    f3 = nyxus_amd.featureset3d
    n = nyxus_amd.Nyxus3DZones(api["features"] + ["*3D_GLCM*", "*3D_NGTDM*"], coarse_gray_depth=64)
    plain = nyxus_amd.Nyxus3D(["*3D_GLCM*", "*3D_NGTDM*"], coarse_gray_depth=64)
    for m in api["metaparams"]:
        n.set_metaparam(m)
        if not m.startswith(("3glrlm", "3glszm")):
            plain.set_metaparam(m)
    df = n.featurize(I, M, intensity_names=["a.vol", "b.vol"], label_names=["a.seg", "b.seg"])
    lead = ["intensity_image", "mask_image", "ROI_label", "t_index"]
    assert list(df.columns) == lead + f3.GLCM_3D + f3.NGTDM_3D + api["columns"]           # Feature3D order: GLSZM, then GLRLM, at the end
    assert list(df["ROI_label"]) == api["labels"] and list(df["intensity_image"]) == [["a.vol", "b.vol"][v] for v in api["volumes"]]
    bad, rel = volzone_cases.compare(df[api["columns"]].to_numpy(), np.array(api["numeric"]), api["columns"])
    print(f"api: largest relative difference {rel:.3e}")
    assert not bad, bad[:10]
    dp = plain.featurize(I, M, intensity_names=["a.vol", "b.vol"], label_names=["a.seg", "b.seg"])
    rest = f3.GLCM_3D + f3.NGTDM_3D
    assert same(df[rest].to_numpy().copy(), dp[rest].to_numpy().copy()).all()             # what Nyxus3D serves has Nyxus3D's bits
    # the defaults leave the 0 .. 2999 intensities unbinned: refused, and the error names the metaparameters
    with pytest.raises(_lib.NyxHipError, match=r'128.*set_metaparam\("3glrlm/greydepth=.*set_metaparam\("3glszm/greydepth=') as ei:
        nyxus_amd.Nyxus3DZones(["*3D_GLRLM*", "*3D_GLSZM*"]).featurize(I, M)
    assert ei.value.code == 4
