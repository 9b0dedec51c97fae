"""The volume entries on the GPU (nyxhip_featurize_volumes, roi_vol.hip): the 36 voxel-intensity columns and the 3-D GLCM columns (30
codes x 13 directions, 29 _AVE) against the values recorded from the reference's own classes (tests/golden/vol) on the cases of
tests/vol_cases.py -- integer-valued and order-statistic columns bit for bit, the rest within parity.REL_TOL (vol_cases.compare) -- the
refusals, and the bits of a row across batch order, memory kind, stated against derived extrema, and chunks.

Largest relative differences printed by test_rows_match_the_reference_classes on an MI355X (DESIGN.md 4.5j records them): intensity
block 4.7e-13, GLCM block 7.7e-12."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import vol_cases
from tests.vol_device import device_rows

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "vol", "vol_reference.npz"))
N_INT = vol_cases.N_INT
ASM_DIR4 = 1 * 13 + 4             # 3GLCM_ASM of direction (1, 0, 0) in the GLCM block: positive wherever that direction has a pair


def same(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def vol_ctx():
    """A context of this module's own on cuda:0: the workspaces these entries grow stay out of the context the other test files share."""
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("bname,mode", vol_cases.CASES)
def test_rows_match_the_reference_classes(vol_ctx, bname, mode):
    b, s = vol_cases.batch(bname), vol_cases.settings(mode)
    want = GOLD[vol_cases.case_name(bname, mode)]
    got = vol_ctx.volumes_host(b, _abi.VFAM_ALL, s)
    bad, ri, rg = vol_cases.compare(got, want)
    print(f"{bname}/{mode}: largest relative difference intensity block {ri:.3e}, GLCM block {rg:.3e}")
    assert not bad, bad[:10]
    # each family alone has the bits it has beside the other
    assert same(vol_ctx.volumes_host(b, _abi.VFAM_INTENSITY, s), got[:, :N_INT]).all()
    assert same(vol_ctx.volumes_host(b, _abi.VFAM_GLCM, s), got[:, N_INT:]).all()


def test_blank_directions_and_soft_nan(vol_ctx):
    b, s = vol_cases.batch("boxes"), vol_cases.settings("softnan")
    T = vol_ctx.volumes_host(b, _abi.VFAM_GLCM, s)[:, :390].reshape(-1, 30, 13)
    blank = (T == s.soft_nan).all(axis=1)
    assert s.soft_nan == -7.5 and blank[0].all()                                        # 1x1x1
    sm = vol_cases.settings("matlab")
    Tm = vol_ctx.volumes_host(b, _abi.VFAM_GLCM, sm)[:, :390].reshape(-1, 30, 13)
    bm = (Tm == 0.0).all(axis=1)
    assert [list(np.flatnonzero(~bm[r])) for r in (1, 2, 3)] == [[4], [10], [12]]        # 2x1x1, 1x2x1, 1x1x2
    assert list(np.flatnonzero(~bm[5])) == [1, 4, 7, 10]                                 # the depth-1 slab


def test_level_cap(vol_ctx):
    b = vol_cases.batch("boxes")
    for g in (vol_cases.LEVEL_CAP, -vol_cases.LEVEL_CAP):                               # exactly at the cap: served
        s = _abi.default_settings(64)
        s.glcm_grey_depth = g
        assert vol_ctx.volumes_host(b, _abi.VFAM_GLCM, s)[4, ASM_DIR4] > 0
    for g in (vol_cases.LEVEL_CAP + 1, -(vol_cases.LEVEL_CAP + 1)):                     # one above: refused, and the message names the cap
        s = _abi.default_settings(64)
        s.glcm_grey_depth = g
        with pytest.raises(_lib.NyxHipError, match=str(vol_cases.LEVEL_CAP)) as ei:
            vol_ctx.volumes_host(b, _abi.VFAM_GLCM, s)
        assert ei.value.code == 4
        vol_ctx.volumes_host(b, _abi.VFAM_INTENSITY, s)                                  # the intensity block does not read the setting
    si = vol_cases.settings("ibsi")
    with pytest.raises(_lib.NyxHipError, match=str(vol_cases.LEVEL_CAP)) as ei:         # IBSI mode: the largest intensity is the level count
        vol_ctx.volumes_host(vol_cases.batch("over"), _abi.VFAM_GLCM, si)
    assert ei.value.code == 4
    with pytest.raises(_lib.NyxHipError) as ei:
        device_rows(vol_ctx, vol_cases.batch("over"), si, _abi.VFAM_GLCM)
    assert ei.value.code == 4
    # the context serves the next call
    assert vol_ctx.volumes_host(b, _abi.VFAM_GLCM, si)[4, ASM_DIR4] > 0


def test_refusals(vol_ctx):
    b, s = vol_cases.batch("boxes"), vol_cases.settings("matlab")
    for mask in (0, 4, 1 << 12, _abi.VFAM_ALL | 8):
        with pytest.raises(_lib.NyxHipError) as ei:
            vol_ctx.volumes_host(b, mask, s)
        assert ei.value.code == 1
    out = np.zeros((b.n_roi, 455))
    cb = b.c_struct()
    import ctypes as C
    assert vol_ctx._lib.nyxhip_featurize_volumes(vol_ctx._h, C.byref(cb), _abi.VFAM_ALL, C.byref(s), out.ctypes.data, 454) == 1   # ld below the columns
    s0 = vol_cases.settings("matlab")
    s0.glcm_offset = 0
    with pytest.raises(_lib.NyxHipError) as ei:
        vol_ctx.volumes_host(b, _abi.VFAM_GLCM, s0)
    assert ei.value.code == 1
    # a box beyond 256^3 cells, and a side beyond 65534
    big = _abi.HostBatch3D(b.roi_label[:1], b.px_offset[:2], b.x[:1], b.y[:1], b.z[:1], b.inten[:1], [257], [256], [256], b.min_inten[:1], b.max_inten[:1])
    with pytest.raises(_lib.NyxHipError, match="256") as ei:
        vol_ctx.volumes_host(big, _abi.VFAM_GLCM, s)
    assert ei.value.code == 5
    long_ = _abi.HostBatch3D(b.roi_label[:1], b.px_offset[:2], b.x[:1], b.y[:1], b.z[:1], b.inten[:1], [65535], [1], [1], b.min_inten[:1], b.max_inten[:1])
    with pytest.raises(_lib.NyxHipError, match="65534") as ei:
        vol_ctx.volumes_host(long_, _abi.VFAM_GLCM, s)
    assert ei.value.code == 5
    # a voxel outside its box is never stored
    out_ = _abi.HostBatch3D(b.roi_label[4:5], [0, 8], b.x[b.px_offset[4]:b.px_offset[5]], b.y[b.px_offset[4]:b.px_offset[5]], b.z[b.px_offset[4]:b.px_offset[5]],
                            b.inten[b.px_offset[4]:b.px_offset[5]], [2], [2], [1], b.min_inten[4:5], b.max_inten[4:5])
    with pytest.raises(_lib.NyxHipError, match="outside its box") as ei:
        vol_ctx.volumes_host(out_, _abi.VFAM_GLCM, s)
    assert ei.value.code == 1
    # a budget that holds no ROI
    with pytest.raises(_lib.NyxHipError, match="max_device_bytes") as ei:
        vol_ctx.volumes_host(vol_cases.batch("blob40"), _abi.VFAM_ALL, s, max_device_bytes=4096)
    assert ei.value.code == 5
    assert vol_ctx.volumes_host(b, _abi.VFAM_ALL, s)[4, N_INT + ASM_DIR4] > 0


def test_an_roi_without_voxels_is_soft_nan(vol_ctx):
    b0, s = vol_cases.batch("boxes"), vol_cases.settings("softnan")
    b = vol_cases.with_empty(b0, at=5)
    got = vol_ctx.volumes_host(b, _abi.VFAM_ALL, s)
    assert (got[5] == s.soft_nan).all()
    assert same(np.delete(got, 5, axis=0), vol_ctx.volumes_host(b0, _abi.VFAM_ALL, s)).all()
    assert same(device_rows(vol_ctx, b, s), got).all()


def test_a_row_has_the_same_bits_however_it_is_asked_for(vol_ctx):
    s = vol_cases.settings("r64")
    parts = [vol_cases.batch(n) for n in ("boxes", "seam", "blob40", "wide")]
    rois = []
    for p in parts:
        rois += [p.select([r]) for r in range(p.n_roi)]
    order = list(range(len(rois)))
    cat = lambda idx: _abi.HostBatch3D(*[np.concatenate([getattr(rois[i], k) for i in idx]) if k != "px_offset" else
                                          np.concatenate([[0], np.cumsum([int(rois[i].px_offset[1]) for i in idx])]).astype(np.uint64)
                                          for k in ("roi_label", "px_offset", "x", "y", "z", "inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten")])
    mixed_b = cat(order)
    mixed = vol_ctx.volumes_host(mixed_b, _abi.VFAM_ALL, s)
    k = 0
    for p in parts:                                                                      # alone | in the mixed batch
        assert same(vol_ctx.volumes_host(p, _abi.VFAM_ALL, s), mixed[k:k + p.n_roi]).all()
        k += p.n_roi
    for r in (0, 4, 8, 12, 13, 14, 15, len(rois) - 1):                                   # single ROIs on both sides of the LDS seam
        assert same(vol_ctx.volumes_host(rois[r], _abi.VFAM_ALL, s), mixed[r:r + 1]).all(), r
    rev = vol_ctx.volumes_host(cat(order[::-1]), _abi.VFAM_ALL, s)                       # reversed batch order
    assert same(rev[::-1], mixed).all()
    assert same(vol_ctx.volumes_host(mixed_b, _abi.VFAM_ALL, s, stated=True), mixed).all()          # stated against derived extrema
    assert same(device_rows(vol_ctx, mixed_b, s, stated=True), mixed).all()              # device memory, stated and derived
    assert same(device_rows(vol_ctx, mixed_b, s, stated=False), mixed).all()
    # chunks: a budget that holds two ROIs' workspaces, then one
    per_roi = 65536 + 2 * 4 * 64000                                                      # the largest box (64000 cells, 256-aligned) + two sort buffers of 38 k voxels at most
    for budget in (2 * per_roi, per_roi):
        assert same(vol_ctx.volumes_host(mixed_b, _abi.VFAM_ALL, s, max_device_bytes=budget), mixed).all(), budget
    assert same(device_rows(vol_ctx, mixed_b, s, max_device_bytes=per_roi), mixed).all()


def test_nyxus3d_featurize_against_the_recording():
    api = json.load(open(os.path.join(HERE, "golden", "vol", "api_expected.json")))
    I, M = vol_cases.api_volumes()
    for key, case in api["cases"].items():
        n = nyxus_amd.Nyxus3D(case["features"], coarse_gray_depth=64)
        df = n.featurize(I, M, intensity_names=["a.vol", "b.vol"], label_names=["a.seg", "b.seg"])
        assert list(df.columns) == ["intensity_image", "mask_image", "ROI_label", "t_index"] + case["columns"], key
        assert list(df["ROI_label"]) == api["labels"] and list(df["intensity_image"]) == [["a.vol", "b.vol"][v] for v in api["volumes"]]
        got = df[case["columns"]].to_numpy()
        bad, ri, rg = vol_cases.compare(got, np.array(case["numeric"]), case["columns"])
        print(f"api/{key}: largest relative difference intensity {ri:.3e}, GLCM {rg:.3e}")
        assert not bad, (key, bad[:10])
    one = nyxus_amd.Nyxus3D(["3MEAN", "3GLCM_ASM_AVE"]).featurize(I[0], M[0])          # a single volume [z, y, x]
    assert list(one["ROI_label"]) == [1, 3, 7] and list(one["intensity_image"]) == ["Intensity0"] * 3
