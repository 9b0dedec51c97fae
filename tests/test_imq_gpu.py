"""The image-quality entries on the GPU (nyxhip_imq_batch / _tiles / _slides, roi_imq.hip): FOCUS_SCORE, LOCAL_FOCUS_SCORE, MAX_SATURATION,
MIN_SATURATION against the values recorded from the reference's own classes (tests/golden/imq) -- the two saturation columns bit for bit,
the two focus columns within parity.REL_TOL and exactly 0 where the recording is 0 -- and the bits of a row across batches, orders,
entries, memories and chunks."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import imq_cases, imq_ref, parity, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = imq_cases.golden()
same = imq_ref.same_bits


@pytest.fixture(scope="module")
def imq_ctx():
    """A context of this module's own on cuda:0: the workspaces, staging slots and table sizes these entries grow stay out of the context
    the other test files share."""
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def check(got, want, tag):
    """Saturation bit for bit; focus within REL_TOL, and an exact 0 where the recording is 0."""
    ok = same(got[:, imq_ref.SATURATION], want[:, imq_ref.SATURATION])
    assert ok.all(), (tag, "saturation", np.argwhere(~ok)[:8].tolist(), got[~ok.all(axis=1)][:4], want[~ok.all(axis=1)][:4])
    rel = imq_ref.rel_diff(got[:, imq_ref.FOCUS], want[:, imq_ref.FOCUS])
    print(f"{tag}: largest relative difference on the focus columns {rel.max():.3e}")
    assert (rel <= parity.REL_TOL).all(), (tag, "focus", float(rel.max()), got[:, imq_ref.FOCUS][rel > parity.REL_TOL][:4], want[:, imq_ref.FOCUS][rel > parity.REL_TOL][:4])


def device_rows(ctx, b, s, stated=True, ld=6):
    import torch
    dev = torch.device("cuda", 0)
    view = {2: np.int16, 4: np.int32, 8: np.int64}
    keep = {k: torch.from_numpy(getattr(b, k).view(view[getattr(b, k).dtype.itemsize])).to(dev)
            for k in ("px_offset", "x", "y", "inten", "bbox_w", "bbox_h", "min_inten", "max_inten")}
    cb = _abi.Batch()
    cb.n_roi = b.n_roi
    for k, t in keep.items():
        setattr(cb, k, t.data_ptr())
    cb.memory = _abi.MEM_DEVICE
    if stated:
        h = b.c_struct()
        cb.max_px, cb.max_bbox_area, cb.max_inten_range, cb.max_bbox_side = h.max_px, h.max_bbox_area, h.max_inten_range, h.max_bbox_side
    out = torch.full((b.n_roi, ld), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.imq_device(cb, s, out.data_ptr(), ld)
    G = out.cpu().numpy()
    assert (G[:, 4:] == -1.0).all()
    return G[:, :4]


@pytest.mark.parametrize("name", list(imq_cases.CASES))
def test_hip_rows_match_the_reference_classes(imq_ctx, name):
    b, s = imq_cases.batch(name), imq_cases.settings()
    host = imq_ctx.imq_host(b, s)
    check(host, GOLD[name], name)
    assert same(device_rows(imq_ctx, b, s), host).all(), name
    assert same(device_rows(imq_ctx, b, s, stated=False), host).all(), name


def test_the_cases_meet_every_launch_form():
    cells = imq_cases.batch("switches").bbox_w.astype(np.int64) * imq_cases.batch("switches").bbox_h
    assert list(cells[:4]) == [imq_cases.WAVE_CELLS, 33 * 32, imq_cases.LDS_CELLS, 121 * 127]
    assert imq_cases.WAVE_CELLS < 33 * 32 <= imq_cases.LDS_CELLS < 121 * 127 and cells[4] > imq_cases.LDS_CELLS
    assert sorted(imq_cases.batch("widths").bbox_w) == [63, 64, 65]


def test_side_1_boxes_against_the_restatement(imq_ctx):
    b, s = imq_cases.batch("side1"), imq_cases.settings()
    assert s.soft_nan != 0 and [(int(w), int(h)) for w, h in zip(b.bbox_w, b.bbox_h)] == [(1, 1), (1, 5), (5, 1)]
    got, want = imq_ctx.imq_host(b, s), imq_ref.table(b, s)
    assert (got[:, 1] == s.soft_nan).all() and (want[:, 1] == s.soft_nan).all()
    assert np.isfinite(got[:, [0, 2, 3]]).all() and not (got[:, [0, 2, 3]] == s.soft_nan).any()
    check(got, want, "side1")
    assert same(device_rows(imq_ctx, b, s), got).all()


def test_empty_rois_are_soft_nan(imq_ctx):
    b0 = imq_cases.batch("filled")
    n0 = int(b0.px_offset[1])
    # ROI 0 loses its pixels; ROI 1 keeps them but its box is empty
    b = _abi.HostBatch(b0.roi_label[:3], np.array([0, 0, int(b0.px_offset[2]) - n0, int(b0.px_offset[3]) - n0]), b0.x[n0:int(b0.px_offset[3])],
                       b0.y[n0:int(b0.px_offset[3])], b0.inten[n0:int(b0.px_offset[3])], np.array([2, 0, 3]), np.array([2, 3, 2]), b0.min_inten[:3], b0.max_inten[:3])
    s = imq_cases.settings()
    got = imq_ctx.imq_host(b, s)
    assert (got[:2] == s.soft_nan).all()
    assert same(got[2:], imq_ctx.imq_host(b0, s)[2:3]).all()


def test_a_row_has_the_same_bits_however_it_is_asked_for(imq_ctx):
    s = imq_cases.settings()
    bm = imq_cases.batch("mixed")
    mixed = imq_ctx.imq_host(bm, s)
    for name in list(imq_cases.CASES) + ["side1"]:                          # alone | in the mixed batch
        k, n = imq_cases.mixed_row(name), imq_cases.batch(name).n_roi
        assert same(imq_ctx.imq_host(imq_cases.batch(name), s), mixed[k:k + n]).all(), name
    rois = [r for n in imq_cases.MIXED_ORDER for r in imq_cases.CASES[n]()] + imq_cases.SIDE1()
    for r in (0, 5, 8, 17, 18, 19, 20, 21, 22, len(rois) - 1):                   # single ROIs of every launch form
        assert same(imq_ctx.imq_host(_abi.batch_from_rois(rois[r:r + 1]), s), mixed[r:r + 1]).all(), r
    rev = imq_ctx.imq_host(_abi.batch_from_rois(rois[::-1]), s)              # reversed ROI order
    assert same(rev[::-1], mixed).all()
    assert same(imq_ctx.imq_host(bm, s), mixed).all()                        # repeatable across calls
    assert same(device_rows(imq_ctx, bm, s), mixed).all() and same(device_rows(imq_ctx, bm, s, stated=False), mixed).all()
    # the same ROIs on a label image, through the tile entry: boxes laid out left to right on one tall-enough tile
    H = int(bm.bbox_h.max()) + 2
    W = int(bm.bbox_w.sum()) + 2 * bm.n_roi
    inten = np.zeros((1, H, W), np.uint32)
    lab = np.zeros((1, H, W), np.uint32)
    x0 = 1
    for r in range(bm.n_roi):
        o, e = int(bm.px_offset[r]), int(bm.px_offset[r + 1])
        inten[0, bm.y[o:e].astype(np.int64) + 1, bm.x[o:e].astype(np.int64) + x0] = bm.inten[o:e]
        lab[0, bm.y[o:e].astype(np.int64) + 1, bm.x[o:e].astype(np.int64) + x0] = r + 1
        x0 += int(bm.bbox_w[r]) + 2
    tiles, labels, T = imq_ctx.imq_tiles_host(inten, lab, s)
    assert list(labels) == list(range(1, bm.n_roi + 1)) and not tiles.any()
    assert same(T, mixed).all(), np.argwhere(~same(T, mixed))[:8].tolist()


def test_tile_entry_and_chunks(imq_ctx):
    s = imq_cases.settings()
    inten, lab = imq_cases.api_tiles()
    b = imq_cases.tile_batch()
    want = imq_ctx.imq_host(b, s)
    check(want, GOLD["tile"], "tile")
    tiles, labels, T = imq_ctx.imq_tiles_host(inten, lab, s)
    assert list(labels) == list(b.roi_label) and list(tiles) == [0, 0, 0, 1, 1] and same(T, want).all()
    tiles, labels, T = imq_ctx.imq_tiles_host(np.concatenate([inten] * 3), np.concatenate([lab] * 3), s, max_device_bytes=1 << 20)
    assert list(tiles) == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 4, 5, 5] and same(T, np.tile(want, (3, 1))).all()


SLIDE_SHAPES = [(2, 2), (7, 3), (64, 64), (129, 257), (300, 70)]            # (w, h); the last: two column blocks x three row strips


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32])
def test_slides_have_the_bits_of_the_batch_entry(imq_ctx, dtype):
    import torch
    s = imq_cases.settings()
    assert 300 > 256 and 70 > 2 * 32                                        # kImqStripCols, kImqStripRows
    for w, h in SLIDE_SHAPES:
        st = np.stack([imq_cases.slide(w, h, dtype, seed=10 * w + k) for k in range(3)])
        if (w, h) == (64, 64):
            st[1][:] = 0                                                     # a slide of zeros: min P == max P
            st[2][:] = 9                                                     # a flat slide
        want = imq_ctx.imq_host(imq_cases.slide_batch(st), s)
        check(want, imq_ref.table(imq_cases.slide_batch(st), s), ("slides, restatement", w, h))
        got = imq_ctx.imq_slides_host(st, s)
        assert same(got, want).all(), ("host", w, h, got, want)
        view = st.view(np.int16) if dtype == np.uint16 else st.view(np.int32) if dtype == np.uint32 else st
        d_in = torch.from_numpy(view).to("cuda:0")
        d_out = torch.full((3, 5), -1.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        imq_ctx.imq_slides_device(d_in.data_ptr(), np.dtype(dtype).itemsize, 3, h, w, s, d_out.data_ptr(), 5)
        G = d_out.cpu().numpy()
        assert same(G[:, :4], want).all() and (G[:, 4] == -1.0).all(), ("device", w, h)
        if (w, h) == (300, 70):                                              # a budget that forces one slide per chunk
            per = 3 * 2 * 18 * 8 + 96 + 2 * st[0].nbytes
            got = imq_ctx.imq_slides_host(st, s, max_device_bytes=per + per // 2)
            assert same(got, want).all(), ("chunks", w, h)


def test_recorded_slides(imq_ctx):
    inten, _ = imq_cases.api_tiles()
    check(imq_ctx.imq_slides_host(inten, imq_cases.settings()), GOLD["slides"], "slides")


def test_error_paths(imq_ctx):
    s = imq_cases.settings()
    lib = _lib.load()
    img = imq_cases.slide(16, 16, np.uint16, 1)[None]
    out = np.zeros(16)
    t = _abi.Tiles()
    t.inten = img.ctypes.data; t.label = img.ctypes.data; t.inten_dtype = _abi.U16; t.width = 16; t.height = 16; t.n_tiles = 1; t.memory = _abi.MEM_HOST
    assert lib.nyxhip_imq_slides(imq_ctx._h, C.byref(t), C.byref(s), out.ctypes.data, 4) == 1
    assert b"label" in lib.nyxhip_last_error(imq_ctx._h)
    t.label = None
    assert lib.nyxhip_imq_slides(imq_ctx._h, C.byref(t), C.byref(s), out.ctypes.data, 3) == 1       # out_ld below the column count
    for w, h in ((65535, 1), (1, 65535), (0, 4), (4, 0)):                    # only the header is validated: nothing of that size exists
        t.width = w; t.height = h
        assert lib.nyxhip_imq_slides(imq_ctx._h, C.byref(t), C.byref(s), out.ctypes.data, 4) == 4
        assert b"whole-slide mode" in lib.nyxhip_last_error(imq_ctx._h)
    t.n_tiles = 0
    assert lib.nyxhip_imq_slides(imq_ctx._h, C.byref(t), C.byref(s), out.ctypes.data, 4) == 0
    assert (out == 0).all()
    # the width bound: 4 * max_inten * n reaches 2^63 -> refused, nothing wraps
    w, h = 65535, 8193                                                       # (2^32 - 1) * w * h >= 2^61; a one-pixel ROI states the box
    b = _abi.HostBatch(np.array([1]), np.array([0, 1]), np.array([0]), np.array([0]), np.array([2 ** 32 - 1]), np.array([w]), np.array([h]),
                       np.array([2 ** 32 - 1]), np.array([2 ** 32 - 1]))
    with pytest.raises(_lib.NyxHipError, match="2\\^63") as ei:
        imq_ctx.imq_host(b, s)
    assert ei.value.code == 4


def test_through_the_image_quality_class(tmp_path):
    api = json.load(open(os.path.join(ROOT, "tests", "golden", "imq", "api_expected.json")))
    inten, lab = imq_cases.api_tiles()
    assert str(inten.dtype) == api["inten_dtype"]

    def agree(got, want, cols):
        assert np.isfinite(got).all()
        for c, col in enumerate(cols):
            if "SATURATION" in col:
                assert (got[:, c] == want[:, c]).all(), col
            else:
                assert (imq_ref.rel_diff(got[:, c], want[:, c]) <= parity.REL_TOL).all(), col

    for case in api["cases"].values():
        df = nyxus_amd.ImageQuality(case["features"]).featurize(inten, lab)
        assert list(df.columns) == ["intensity_image", "mask_image", "ROI_label", "t_index"] + case["columns"]
        assert list(df["ROI_label"]) == api["labels"]
        assert list(df["intensity_image"]) == ["Intensity%d" % t for t in api["tiles"]]
        agree(df[case["columns"]].values.astype(float), np.array(case["numeric"]), case["columns"])
    # whole images: featurize_files(..., single_roi=True) and a directory without labels
    d = tmp_path / "int"
    d.mkdir()
    paths = []
    for k in range(inten.shape[0]):
        paths.append(str(d / ("slide%d.tif" % k)))
        synth.write_tiled_tiff(paths[-1], inten[k], tile=32)
    case = api["single_roi"]
    iq = nyxus_amd.ImageQuality(case["features"])
    for df in (iq.featurize_files(paths, None, True), iq.featurize_directory(str(d))):
        assert list(df.columns[4:]) == case["columns"] and list(df["intensity_image"]) == paths
        assert (df["ROI_label"] == 1).all() and (df["mask_image"] == "").all()
        agree(df[case["columns"]].values.astype(float), np.array(case["numeric"]), case["columns"])
