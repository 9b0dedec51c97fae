"""The volume distance-zone entry on the GPU (nyxhip_featurize_volumes_dzones, roi_voldzone.hip): the 18 GLDZM columns against the values
recorded from the reference's own class (tests/golden/voldzone) and against tests/voldzone_ref.py, both within TOL; the `rule` batch
against the restatement, which is all the reference leaves defined there; the edge and seam cases, the level cap, the refusals, and
the bits of a row across batch order, memory kind, stated against derived extrema and chunks.

TOL is the bound tests/test_volzone_gpu.py and tests/test_voltex_gpu.py use.  The integer matrix agrees exactly; what differs between the
kernel's closing and the other two is the order of the fp64 sums (a lane sums its distances and the lanes are added in lane order) and the
last bit of log2.  tests/test_voldzone_cpu.py shows that one moved count moves a column by more than 10 x TOL.  The variance columns (GLV,
ZDV) are measured against max(|value|, 1) (voldzone_cases.floor).  A call that returns has found the device status word 0: the entry
checks it after the stream has drained and fails otherwise."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import voldzone_cases, voldzone_edge_cases, voldzone_ref
from tests.voldzone_device import device_rows

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "voldzone", "voldzone_reference.npz"))
TOL = 1e-10
DZ = _abi.VDZ_GLDZM


def same(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def held(got, want, label):
    """NaN / inf in the same places, finite values within TOL; prints the largest relative difference before it asserts"""
    rel = voldzone_cases.rel_diff(got, want)
    print(f"{label}: largest relative difference {rel[np.isfinite(rel)].max(initial=0.0):.3e}")
    assert (np.isnan(got) == np.isnan(want)).all() and (np.isinf(got) == np.isinf(want)).all(), label
    assert (rel <= TOL).all(), (label, [(int(r), voldzone_cases.NAMES[c], got[r, c], want[r, c]) for r, c in np.argwhere(~(rel <= TOL))[:5]])


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own on cuda:0: the workspaces these entries grow stay out of the context the other test files share."""
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("bname,mode", voldzone_cases.CASES)
def test_rows_match_the_reference_class(ctx, bname, mode):
    b = voldzone_cases.batch(bname)
    s = voldzone_cases.settings(mode)
    assert not voldzone_cases.rule_excluded(b, s).any()
    got = ctx.volumes_dzones_host(b, DZ, s)
    held(got, GOLD[voldzone_cases.case_name(bname, mode)], f"{bname}/{mode} vs the recording")
    held(got, voldzone_ref.table(b, s), f"{bname}/{mode} vs the restatement")


@pytest.mark.parametrize("bname,mode", voldzone_cases.RULE_CASES)
def test_the_rule_batch_against_the_restatement(ctx, bname, mode):
    b = voldzone_cases.batch(bname)
    s = voldzone_cases.settings(mode)
    assert voldzone_cases.rule_excluded(b, s).sum() == b.n_roi - 1      # every ROI but the flat one
    got = ctx.volumes_dzones_host(b, DZ, s)
    held(got, voldzone_ref.table(b, s), f"{bname}/{mode} vs the restatement")
    held(got, GOLD[voldzone_cases.case_name(bname, mode) + "__restated"], f"{bname}/{mode} vs the stored restatement")
    assert same(device_rows(ctx, b, s), got).all()


@pytest.mark.parametrize("case", voldzone_edge_cases.cases(), ids=lambda c: c[0])
def test_edge_and_seam_rows_against_the_restatement(ctx, case):
    name, b, s = case
    got = ctx.volumes_dzones_host(b, DZ, s)
    held(got, voldzone_ref.table(b, s), name)
    assert same(device_rows(ctx, b, s), got).all()
    if name == "degenerate":
        flat = (b.counts() == 0) | (b.max_inten == b.min_inten)
        assert flat.sum() == 4 and (got[flat] == s.soft_nan).all() and np.isfinite(got[~flat]).all()


def test_level_cap_host_and_device(ctx):
    b = voldzone_cases.batch("full")
    cap = voldzone_cases.LEVEL_CAP
    for v in (cap, -cap):                                                                 # exactly at the cap: served
        s = voldzone_cases.settings("matlab")
        s.grey_depth = v
        assert np.isfinite(ctx.volumes_dzones_host(b, DZ, s)[8]).all()
    for v in (cap + 1, -(cap + 1)):
        s = voldzone_cases.settings("matlab")
        s.grey_depth = v
        with pytest.raises(_lib.NyxHipError, match=str(cap) + ".*coarse_gray_depth") as ei:
            ctx.volumes_dzones_host(b, DZ, s)
        assert ei.value.code == _abi.ERR_UNSUPPORTED
        s.ibsi = 1                                                                        # IBSI mode does not read it
        assert np.isfinite(ctx.volumes_dzones_host(b, DZ, s)[8]).all()
    # IBSI mode / grey depth 0: the largest intensity of an ROI is the level count -- found on the device, with a good ROI beside it
    def one(v):
        z, y, x = np.meshgrid(np.arange(2), np.arange(2), np.arange(3), indexing="ij")
        return {"x": x.ravel(), "y": y.ravel(), "z": z.ravel(), "inten": np.r_[np.arange(1, 12), v].astype(np.uint32), "origin": (0, 0, 0), "box": (3, 2, 2)}
    at, over = _abi.batch3d_from_rois([one(cap)]), _abi.batch3d_from_rois([one(5), one(cap + 1)])
    for mode in ("ibsi", "none"):
        s = voldzone_cases.settings(mode)
        held(ctx.volumes_dzones_host(at, DZ, s), voldzone_ref.table(at, s), f"128 levels, {mode}")
        with pytest.raises(_lib.NyxHipError, match=str(cap) + ".*coarse_gray_depth") as ei:
            ctx.volumes_dzones_host(over, DZ, s)
        assert ei.value.code == _abi.ERR_UNSUPPORTED
    with pytest.raises(_lib.NyxHipError) as ei:
        device_rows(ctx, over, voldzone_cases.settings("ibsi"))
    assert ei.value.code == _abi.ERR_UNSUPPORTED
    s = voldzone_cases.settings("radiomics")                                              # the context serves the next call
    assert same(ctx.volumes_dzones_host(over.select([0]), DZ, s), ctx.volumes_dzones_host(over, DZ, s)[:1]).all()


def test_refusals(ctx):
    b = voldzone_cases.batch("full")
    s = voldzone_cases.settings("matlab")
    for mask in (0, 2, 1 << 12):
        with pytest.raises(_lib.NyxHipError) as ei:
            ctx.volumes_dzones_host(b, mask, s)
        assert ei.value.code == 1
        assert ctx._lib.nyxhip_voldzone_n_columns(mask) < 0
    import ctypes as C
    out = np.zeros((b.n_roi, 18))
    cb = b.c_struct()
    assert ctx._lib.nyxhip_featurize_volumes_dzones(ctx._h, C.byref(cb), DZ, C.byref(s), out.ctypes.data, 17) == 1     # ld below the columns
    assert ctx._lib.nyxhip_featurize_volumes_dzones(ctx._h, C.byref(cb), DZ, None, out.ctypes.data, 18) == 1
    o4, o5 = int(b.px_offset[4]), int(b.px_offset[5])
    out_ = _abi.HostBatch3D(b.roi_label[4:5], [0, o5 - o4], b.x[o4:o5], b.y[o4:o5], b.z[o4:o5], b.inten[o4:o5], [2], [2], [1], b.min_inten[4:5], b.max_inten[4:5])
    with pytest.raises(_lib.NyxHipError, match="outside its box") as ei:
        ctx.volumes_dzones_host(out_, DZ, s)
    assert ei.value.code == 1
    with pytest.raises(_lib.NyxHipError, match="max_device_bytes") as ei:
        ctx.volumes_dzones_host(b, DZ, s, max_device_bytes=64)
    assert ei.value.code == 5
    assert _lib.voldzone_column_names(DZ) == voldzone_cases.column_names()
    assert np.isfinite(ctx.volumes_dzones_host(b, DZ, s)[8]).all()                        # the context serves the next call


def test_a_row_has_the_same_bits_however_it_is_asked_for(ctx):
    s = voldzone_cases.settings("none")
    E = {c[0]: c[1] for c in voldzone_edge_cases.cases()}
    parts = [voldzone_cases.batch(n) for n in ("boxes", "full", "conn")] + [E["wg"].select([0, 3, 10]), E["emit"]]
    rois = []
    for p in parts:
        rois += [p.select([r]) for r in range(p.n_roi)]
    order = list(range(len(rois)))
    cat = lambda idx: _abi.HostBatch3D(*[np.concatenate([getattr(rois[i], k) for i in idx]) if k != "px_offset" else
                                          np.concatenate([[0], np.cumsum([int(rois[i].px_offset[1]) for i in idx])]).astype(np.uint64)
                                          for k in ("roi_label", "px_offset", "x", "y", "z", "inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten")])
    mixed_b = cat(order)
    mixed = ctx.volumes_dzones_host(mixed_b, DZ, s)
    held(mixed, voldzone_ref.table(mixed_b, s), "mixed")
    k = 0
    for p in parts:                                                                      # alone | in the mixed batch
        assert same(ctx.volumes_dzones_host(p, DZ, s), mixed[k:k + p.n_roi]).all()
        k += p.n_roi
    for r in (0, 4, 11, 16, 20, 25, len(rois) - 4, len(rois) - 1):                        # single ROIs: a launch sized by the ROI alone
        assert same(ctx.volumes_dzones_host(rois[r], DZ, s), mixed[r:r + 1]).all(), r
    assert same(ctx.volumes_dzones_host(cat(order[::-1]), DZ, s)[::-1], mixed).all()      # reversed batch order
    assert same(ctx.volumes_dzones_host(mixed_b, DZ, s, stated=True), mixed).all()        # stated against derived extrema
    assert same(device_rows(ctx, mixed_b, s, stated=True), mixed).all()                   # device memory, stated and derived
    assert same(device_rows(ctx, mixed_b, s, stated=False), mixed).all()
    # chunks: budgets that hold a few ROIs' workspaces, then exactly one
    with pytest.raises(_lib.NyxHipError, match=r"one ROI \((\d+) bytes\)") as ei:
        ctx.volumes_dzones_host(mixed_b, DZ, s, max_device_bytes=64)
    per_roi = int(str(ei.value).split("one ROI (")[1].split(" bytes")[0])
    for budget in (3 * per_roi + 5, per_roi):
        assert same(ctx.volumes_dzones_host(mixed_b, DZ, s, max_device_bytes=budget), mixed).all(), budget
    assert same(device_rows(ctx, mixed_b, s, max_device_bytes=2 * per_roi), mixed).all()


def test_nyxus3ddistancezones_featurize_against_the_recording():
    api = json.load(open(os.path.join(HERE, "golden", "voldzone", "api_expected.json")))
    I, M = voldzone_cases.api_volumes()
    f3 = nyxus_amd.featureset3d
    n = nyxus_amd.Nyxus3DDistanceZones(api["features"] + ["*3D_GLDM*", "*3D_NGLDM*", "3GLSZM_ZP"], coarse_gray_depth=api["coarse_gray_depth"])
    zones = nyxus_amd.Nyxus3DZones(["*3D_GLDM*", "*3D_NGLDM*", "3GLSZM_ZP"], coarse_gray_depth=api["coarse_gray_depth"])
    for m in ("3gldm/greydepth=64", "3glszm/greydepth=12"):
        n.set_metaparam(m)
        zones.set_metaparam(m)
    df = n.featurize(I, M, intensity_names=["a.vol", "b.vol"], label_names=["a.seg", "b.seg"])
    lead = ["intensity_image", "mask_image", "ROI_label", "t_index"]
    assert list(df.columns) == lead + f3.GLDM_3D + api["columns"] + f3.NGLDM_3D + ["3GLSZM_ZP"]   # Feature3D order: GLDZM between GLDM and NGLDM
    assert list(df["ROI_label"]) == api["labels"] and list(df["intensity_image"]) == [["a.vol", "b.vol"][v] for v in api["volumes"]]
    held(df[api["columns"]].to_numpy(), np.array(api["numeric"]), "api")
    dz = zones.featurize(I, M, intensity_names=["a.vol", "b.vol"], label_names=["a.seg", "b.seg"])
    rest = f3.GLDM_3D + f3.NGLDM_3D + ["3GLSZM_ZP"]
    assert same(df[rest].to_numpy().copy(), dz[rest].to_numpy().copy()).all()             # what Nyxus3DZones serves has its bits
    only = nyxus_amd.Nyxus3DDistanceZones(["3GLDZM_ZP", "3gldzm_sde"], coarse_gray_depth=api["coarse_gray_depth"]).featurize(I, M)
    assert list(only.columns) == lead + ["3GLDZM_SDE", "3GLDZM_ZP"]
    assert same(only[["3GLDZM_SDE", "3GLDZM_ZP"]].to_numpy().copy(), df[["3GLDZM_SDE", "3GLDZM_ZP"]].to_numpy().copy()).all()
