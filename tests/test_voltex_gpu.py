"""The volume texture entry on the GPU (nyxhip_featurize_volumes_tex, roi_voltex.hip): the 14 GLDM, 19 NGLDM and 5 NGTDM columns against
the values recorded from the reference's own classes (tests/golden/voltex) under the project's policy (voltex_cases.compare:
parity.REL_TOL), the edge and seam cases against tests/voltex_ref.py within SEAM_TOL, the refusals, and the bits of a row across batch
order, memory kind, stated against derived extrema, and chunks.

SEAM_TOL.  The tables are integers and agree exactly; what differs between the kernel's closing and the restatement is the order of the
fp64 sums (the kernel follows the reference's loops, NumPy sums pairwise) and the last bit of log().  The largest relative difference
test_edge_and_seam_rows_against_the_restatement printed on an MI355X is in DESIGN.md 4.5k; SEAM_TOL lies more than 100 x above it, and
tests/test_voltex_cpu.py shows that one lost count moves a column by more than 10 x SEAM_TOL.  The four variance columns (3GLDM_GLV,
3GLDM_DV, 3NGLDM_GLV, 3NGLDM_DCV) are sums of p (x - mu)^2 over levels or dependence counts x >= 1: where all the mass sits on one x the
exact value is 0 and either side may land on rounding noise of mu, so for them the difference is measured against max(|value|, 1), the
size of the smallest term that cancels."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import voltex_cases, voltex_edge_cases, voltex_ref
from tests.voltex_device import device_rows

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "voltex", "voltex_reference.npz"))
SEAM_TOL = 1e-10
G, N, T = voltex_cases.N_GLDM, voltex_cases.N_NGLDM, voltex_cases.N_NGTDM
ALL = _abi.VTEX_ALL
FLOOR = np.array([1.0 if c in ("3GLDM_GLV", "3GLDM_DV", "3NGLDM_GLV", "3NGLDM_DCV") else 0.0 for c in voltex_cases.column_names()])


def same(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own on cuda:0: the workspaces these entries grow stay out of the context the other test files share."""
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("bname,mode", voltex_cases.CASES)
def test_rows_match_the_reference_classes(ctx, bname, mode):
    b = voltex_cases.batch(bname)
    s, t = voltex_cases.settings(mode)
    want = GOLD[voltex_cases.case_name(bname, mode)]
    got = ctx.volumes_tex_host(b, ALL, s, t)
    bad, rel = voltex_cases.compare(got, want)
    print(f"{bname}/{mode}: largest relative difference {rel:.3e}")
    assert not bad, bad[:10]
    # each class alone has the bits it has beside the others
    assert same(ctx.volumes_tex_host(b, _abi.VTEX_GLDM, s, t), got[:, :G]).all()
    assert same(ctx.volumes_tex_host(b, _abi.VTEX_NGLDM, s, t), got[:, G:G + N]).all()
    assert same(ctx.volumes_tex_host(b, _abi.VTEX_NGTDM, s, t), got[:, G + N:]).all()
    assert same(ctx.volumes_tex_host(b, _abi.VTEX_GLDM | _abi.VTEX_NGTDM, s, t), np.hstack([got[:, :G], got[:, G + N:]])).all()


@pytest.mark.parametrize("case", voltex_edge_cases.cases() + [("seam", voltex_cases.batch("seam"), *voltex_cases.settings("rad64"))], ids=lambda c: c[0])
def test_edge_and_seam_rows_against_the_restatement(ctx, case):
    name, b, s, t = case
    want = voltex_ref.table(b, s, t)
    got = ctx.volumes_tex_host(b, ALL, s, t)
    assert (np.isnan(got) == np.isnan(want)).all() and (np.isinf(got) == np.isinf(want)).all()
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(fin & (want != got), np.abs(got - want) / np.maximum(np.abs(want), FLOOR[None, :]), 0.0)
    print(f"{name}: largest relative difference GPU vs restatement {np.nanmax(rel):.3e}")
    assert (rel <= SEAM_TOL).all(), (name, np.argwhere(rel > SEAM_TOL)[:5].tolist())
    assert same(device_rows(ctx, b, s, t), got).all()


def test_level_cap_and_radius(ctx):
    b = voltex_cases.batch("boxes")
    s, t = voltex_cases.settings("cap")                                                 # exactly at the cap: served
    assert np.isfinite(ctx.volumes_tex_host(b, ALL, s, t)[11]).all()
    cap = str(voltex_cases.LEVEL_CAP)
    for field, bit, pat in (("gldm_grey_depth", _abi.VTEX_GLDM, "gldm_grey_depth"), ("ngtdm_grey_depth", _abi.VTEX_NGTDM, "ngtdm_grey_depth")):
        for v in (voltex_cases.LEVEL_CAP + 1, -(voltex_cases.LEVEL_CAP + 1)):
            s, t = voltex_cases.settings("radiomics")
            setattr(t, field, v)
            with pytest.raises(_lib.NyxHipError, match=cap + ".*" + pat) as ei:
                ctx.volumes_tex_host(b, ALL, s, t)
            assert ei.value.code == 4
            assert np.isfinite(ctx.volumes_tex_host(b, ALL & ~bit, s, t)[11]).all()      # the other classes do not read the setting
    s, t = voltex_cases.settings("radiomics")
    for gd in (voltex_cases.LEVEL_CAP + 1, -1):                                          # NGLDM reads grey_depth as unsigned
        s.grey_depth = gd
        with pytest.raises(_lib.NyxHipError, match=cap + ".*grey_depth") as ei:
            ctx.volumes_tex_host(b, _abi.VTEX_NGLDM, s, t)
        assert ei.value.code == 4
    # IBSI mode / grey depth 0: the largest intensity of an ROI is the level count -- found on the device, with a good ROI beside it
    over = voltex_cases.batch("over")
    both = _abi.batch3d_from_rois([{"x": q.x, "y": q.y, "z": q.z, "inten": q.inten, "origin": (0, 0, 0), "box": (int(q.bbox_w[0]), int(q.bbox_h[0]), int(q.bbox_d[0]))}
                                   for q in (b.select([11]), over)])
    si, ti = voltex_cases.settings("ibsi")
    s0, t0 = voltex_cases.settings("radiomics")
    t0.gldm_grey_depth = t0.ngtdm_grey_depth = 0
    for bit in (_abi.VTEX_GLDM, _abi.VTEX_NGLDM, _abi.VTEX_NGTDM):
        with pytest.raises(_lib.NyxHipError, match=cap) as ei:
            ctx.volumes_tex_host(both, bit, si, ti)
        assert ei.value.code == 4
    for bit in (_abi.VTEX_GLDM, _abi.VTEX_NGTDM):
        with pytest.raises(_lib.NyxHipError, match=cap) as ei:
            ctx.volumes_tex_host(both, bit, s0, t0)
        assert ei.value.code == 4
    with pytest.raises(_lib.NyxHipError) as ei:
        device_rows(ctx, both, si, ti)
    assert ei.value.code == 4
    # radius 0 needs no level table: the cap does not apply to the NGTDM block
    t0.ngtdm_radius = 0
    r0 = ctx.volumes_tex_host(both, _abi.VTEX_NGTDM, s0, t0)
    assert np.isnan(r0).all()
    for rad in (-1, voltex_cases._abi.VOLTEX_MAX_RADIUS + 1):
        s, t = voltex_cases.settings("radiomics")
        t.ngtdm_radius = rad
        with pytest.raises(_lib.NyxHipError, match="ngtdm_radius") as ei:
            ctx.volumes_tex_host(b, ALL, s, t)
        assert ei.value.code == 4
        assert np.isfinite(ctx.volumes_tex_host(b, _abi.VTEX_GLDM, s, t)[11]).all()
    # the context serves the next call
    s, t = voltex_cases.settings("radiomics")
    assert same(ctx.volumes_tex_host(b.select([11]), ALL, s, t), ctx.volumes_tex_host(both, ALL, s, t)[:1]).all()


def test_refusals(ctx):
    b = voltex_cases.batch("boxes")
    s, t = voltex_cases.settings("matlab")
    for mask in (0, 8, 1 << 12, ALL | 8):
        with pytest.raises(_lib.NyxHipError) as ei:
            ctx.volumes_tex_host(b, mask, s, t)
        assert ei.value.code == 1
    import ctypes as C
    out = np.zeros((b.n_roi, 38))
    cb = b.c_struct()
    assert ctx._lib.nyxhip_featurize_volumes_tex(ctx._h, C.byref(cb), ALL, C.byref(s), C.byref(t), out.ctypes.data, 37) == 1     # ld below the columns
    assert ctx._lib.nyxhip_featurize_volumes_tex(ctx._h, C.byref(cb), ALL, C.byref(s), None, out.ctypes.data, 38) == 1
    big = _abi.HostBatch3D(b.roi_label[:1], b.px_offset[:2], b.x[:1], b.y[:1], b.z[:1], b.inten[:1], [257], [256], [256], b.min_inten[:1], b.max_inten[:1])
    with pytest.raises(_lib.NyxHipError, match="256") as ei:
        ctx.volumes_tex_host(big, ALL, s, t)
    assert ei.value.code == 5
    o4, o5 = int(b.px_offset[4]), int(b.px_offset[5])
    out_ = _abi.HostBatch3D(b.roi_label[4:5], [0, 8], b.x[o4:o5], b.y[o4:o5], b.z[o4:o5], b.inten[o4:o5], [2], [2], [1], b.min_inten[4:5], b.max_inten[4:5])
    for bit in (_abi.VTEX_GLDM, _abi.VTEX_NGLDM, _abi.VTEX_NGTDM):
        with pytest.raises(_lib.NyxHipError, match="outside its box") as ei:
            ctx.volumes_tex_host(out_, bit, s, t)
        assert ei.value.code == 1
    t.ngtdm_radius = 0
    with pytest.raises(_lib.NyxHipError, match="outside its box"):
        ctx.volumes_tex_host(out_, _abi.VTEX_NGTDM, s, t)
    with pytest.raises(_lib.NyxHipError, match="max_device_bytes") as ei:
        ctx.volumes_tex_host(voltex_cases.batch("blob40"), ALL, s, t, max_device_bytes=4096)
    assert ei.value.code == 5


def test_an_roi_without_voxels_is_soft_nan(ctx):
    b0 = voltex_cases.batch("boxes")
    b = voltex_cases.with_empty(b0, at=5)
    for mode in ("softnan", "r0"):
        s, t = voltex_cases.settings(mode)
        s.soft_nan = -7.5
        got = ctx.volumes_tex_host(b, ALL, s, t)
        assert (got[5] == -7.5).all()
        assert same(np.delete(got, 5, axis=0), ctx.volumes_tex_host(b0, ALL, s, t)).all()
        assert same(device_rows(ctx, b, s, t), got).all()


def test_a_row_has_the_same_bits_however_it_is_asked_for(ctx):
    s, t = voltex_cases.settings("r2")                                                   # two binned boxes, radius 2
    parts = [voltex_cases.batch(n) for n in ("boxes", "seam", "blob40", "wide")] + [voltex_edge_cases.cases()[1][1]]
    rois = []
    for p in parts:
        rois += [p.select([r]) for r in range(p.n_roi)]
    order = list(range(len(rois)))
    cat = lambda idx: _abi.HostBatch3D(*[np.concatenate([getattr(rois[i], k) for i in idx]) if k != "px_offset" else
                                          np.concatenate([[0], np.cumsum([int(rois[i].px_offset[1]) for i in idx])]).astype(np.uint64)
                                          for k in ("roi_label", "px_offset", "x", "y", "z", "inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten")])
    mixed_b = cat(order)
    mixed = ctx.volumes_tex_host(mixed_b, ALL, s, t)
    k = 0
    for p in parts:                                                                      # alone | in the mixed batch
        assert same(ctx.volumes_tex_host(p, ALL, s, t), mixed[k:k + p.n_roi]).all()
        k += p.n_roi
    for r in (0, 4, 8, 12, 13, 14, 15, len(rois) - 1):                                   # single ROIs: a launch sized by the ROI alone
        assert same(ctx.volumes_tex_host(rois[r], ALL, s, t), mixed[r:r + 1]).all(), r
    assert same(ctx.volumes_tex_host(cat(order[::-1]), ALL, s, t)[::-1], mixed).all()   # reversed batch order
    assert same(ctx.volumes_tex_host(mixed_b, ALL, s, t, stated=True), mixed).all()      # stated against derived extrema
    assert same(device_rows(ctx, mixed_b, s, t, stated=True), mixed).all()               # device memory, stated and derived
    assert same(device_rows(ctx, mixed_b, s, t, stated=False), mixed).all()
    # chunks: a budget that holds two ROIs' workspaces, then one (three boxes of the largest ROI, 65538 cells, and the three tables)
    per_roi = 3 * 65792 + 14080 + 13056 + 4 * (138 + 2 * 129 * 27) + 1024
    for budget in (2 * per_roi, per_roi):
        assert same(ctx.volumes_tex_host(mixed_b, ALL, s, t, max_device_bytes=budget), mixed).all(), budget
    assert same(device_rows(ctx, mixed_b, s, t, max_device_bytes=per_roi), mixed).all()


def test_ngtdm_at_radius_0_alone_takes_no_workspace_and_keeps_its_bits(ctx):
    """NGTDM alone at radius 0 has neither a box nor a table: no workspace, so no budget is read and a budget of one byte serves it.
    Its five columns carry the bits they have in the table of the whole mask: NaN without a zone, soft_nan below two levels."""
    s, t = voltex_cases.settings("r0")
    for bname in ("wide", "boxes"):                                                      # the smallest batch of more than one ROI; rows of both kinds
        b = voltex_cases.batch(bname)
        want = ctx.volumes_tex_host(b, ALL, s, t)[:, G + N:]
        for budget in (0, 1):
            assert same(ctx.volumes_tex_host(b, _abi.VTEX_NGTDM, s, t, max_device_bytes=budget), want).all(), (bname, budget)
            assert same(device_rows(ctx, b, s, t, tmask=_abi.VTEX_NGTDM, max_device_bytes=budget), want).all(), (bname, budget)
        with pytest.raises(_lib.NyxHipError, match="max_device_bytes"):                  # (the whole mask does take a workspace)
            ctx.volumes_tex_host(b, ALL, s, t, max_device_bytes=1)
    assert np.isnan(want).any() and (want == s.soft_nan).any()


def test_nyxus3d_featurize_against_the_recording():
    api = json.load(open(os.path.join(HERE, "golden", "voltex", "api_expected.json")))
    I, M = voltex_cases.api_volumes()
    for key, case in api["cases"].items():
        n = nyxus_amd.Nyxus3D(case["features"] + (["*3D_GLCM*"] if key == "set" else []), coarse_gray_depth=64)
        for m in case["metaparams"]:
            n.set_metaparam(m)
        df = n.featurize(I, M, intensity_names=["a.vol", "b.vol"], label_names=["a.seg", "b.seg"])
        lead = ["intensity_image", "mask_image", "ROI_label", "t_index"] + (nyxus_amd.featureset3d.GLCM_3D if key == "set" else [])
        assert list(df.columns) == lead + case["columns"], key                           # Feature3D order: behind the GLCM
        assert list(df["ROI_label"]) == api["labels"] and list(df["intensity_image"]) == [["a.vol", "b.vol"][v] for v in api["volumes"]]
        bad, rel = voltex_cases.compare(df[case["columns"]].to_numpy(), np.array(case["numeric"]), case["columns"])
        print(f"api/{key}: largest relative difference {rel:.3e}")
        assert not bad, (key, bad[:10])
        if key == "defaults":                                                            # radius 0: NGTDM is soft_nan in the DataFrame
            assert (df[nyxus_amd.featureset3d.NGTDM_3D].to_numpy() == n._settings.soft_nan).all()
    # the defaults leave the 0 .. 2999 intensities unbinned: GLDM is refused, and the error names the metaparameter
    with pytest.raises(_lib.NyxHipError, match=r'128.*set_metaparam\("3gldm/greydepth=') as ei:
        nyxus_amd.Nyxus3D(["*3D_GLDM*"]).featurize(I, M)
    assert ei.value.code == 4
