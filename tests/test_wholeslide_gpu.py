"""Whole-slide mode on the device (nyxhip_featurize_slides): row t of the table has the bits of nyxhip_featurize_batch on the one-ROI
batch tests/wholeslide_cases.slide_batch builds from slide t -- on either side of every choice the entry makes (the chain for dense
slides of the largest size class, the cloud route for everything else) -- and agrees with the oracle under tests/parity.py."""
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import parity, synth
from tests import wholeslide_cases as wc

pytestmark = pytest.mark.gpu

INT, GLCM = _abi.FAM_INTENSITY, _abi.FAM_GLCM


def _or_code(f):
    try:
        return f()
    except _lib.NyxHipError as e:
        return e.code


def _assert_same(got, want, what):
    """Tables with the same bits (NaN equals NaN), or the same error code on both sides."""
    if isinstance(got, int) or isinstance(want, int):
        assert isinstance(got, int) and isinstance(want, int) and got == want, (what, got if isinstance(got, int) else "table", want if isinstance(want, int) else "table")
        return
    assert got.shape == want.shape, what
    ok = wc.same_bits(got, want)
    assert ok.all(), (what, [(int(r), int(c), got[r, c], want[r, c]) for r, c in np.argwhere(~ok)[:6]])


def _invariant(ctx, imgs, mask, s, what, rows=None):
    """featurize_slides_host on the stack against featurize_host on slide_batch of the same slides (rows: the slides to compare)."""
    got = _or_code(lambda: ctx.featurize_slides_host(np.stack(imgs), mask, s))
    rows = range(len(imgs)) if rows is None else rows
    want = _or_code(lambda: ctx.featurize_host(wc.slide_batch([imgs[r] for r in rows]), mask, s))
    if not isinstance(got, int):
        got = got[list(rows)]
    _assert_same(got, want, what)


def _masks(sname):
    return (GLCM, INT | GLCM) if sname == "sub2" else (INT, GLCM, INT | GLCM)


@pytest.mark.parametrize("shape", wc.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_rows_have_the_bits_of_the_batch_entry(hip_ctx, shape):
    w, h = shape
    for dt in wc.DTYPES:
        if shape == (259, 127) and dt != np.uint8:
            continue                                                        # (the shape exists for its unaligned 8-bit rows)
        for sname, kind in wc.CASES + (wc.CASES_U32 if dt == np.uint32 else []):
            s = wc.settings(sname)
            img = wc.slide(w, h, dt, kind)
            for mask in _masks(sname):
                _invariant(hip_ctx, [img], mask, s, (shape, np.dtype(dt).name, sname, kind, mask))


def test_a_slide_whose_base_is_not_aligned(hip_ctx):
    """259 x 127 of uint8 in the middle of a stack of three: its first pixel sits at an odd byte."""
    imgs = [wc.slide(259, 127, np.uint8, "random", seed=k) for k in range(3)]
    assert (259 * 127) % 16 != 0
    for sname in ("gd8", "gd64", "gdm16", "ibsi", "gd300", "sub2"):
        if sname == "ibsi":
            imgs_s = [wc.slide(259, 127, np.uint8, "ibsi", seed=k) for k in range(3)]
        else:
            imgs_s = imgs
        for mask in _masks(sname):
            _invariant(hip_ctx, imgs_s, mask, wc.settings(sname), (sname, mask), rows=[1])
            _invariant(hip_ctx, imgs_s, mask, wc.settings(sname), (sname, mask, "all"))


_ORACLE_CASES = [("gd8", "random"), ("gd64", "zeros"), ("ibsi", "ibsi")]


@pytest.mark.parametrize("shape", wc.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_rows_agree_with_the_oracle(hip_ctx, shape):
    w, h = shape
    mask = INT | GLCM
    for sname, kind in _ORACLE_CASES:
        s = wc.settings(sname)
        names = _lib.column_names(mask, s)
        imgs = [wc.slide(w, h, dt, kind) for dt in wc.DTYPES]
        b = wc.slide_batch(imgs)
        want = po.oracle_featurize(b, mask, s)
        got = np.vstack([hip_ctx.featurize_slides_host(img[None], mask, s) for img in imgs])
        bad = parity.compare_tables(got, want, names, batch=b)
        assert not bad, (shape, sname, bad[:8])
        assert (got[:, names.index("COVERED_IMAGE_INTENSITY_RANGE")] == 1.0).all()
        if shape in ((257, 33), (181, 182)) and po.have_ref():              # ... and with the reference's own classes, where they are built
            bad = parity.compare_tables(got, po.ref_featurize(b, mask, s), names, batch=b)
            assert not bad, (shape, sname, "reference classes", bad[:8])


def test_which_chain_takes_a_slide(hip_ctx):
    """The dense chain (launch report: cooperative bits 0 and 3) takes INTENSITY / GLCM on slides of the largest size class whose range
    is below 2^22; everything else goes through clouds.  A function of the slide and the mask: a stack that mixes both gets both."""
    s = wc.settings("gd64")

    def dense(img, mask):
        hip_ctx.featurize_slides_host(img[None] if img.ndim == 2 else img, mask, s)
        return [bool(r["cooperative"] & 8) for r in hip_ctx.launch_report()]

    for shape in wc.DENSE_SHAPES:
        for dt in wc.DTYPES:
            for mask in (INT, GLCM, INT | GLCM):
                assert dense(wc.slide(*shape, dt), mask) == [True], (shape, dt, mask)
    assert hip_ctx.launch_report()[0]["cooperative"] == 9 and hip_ctx.launch_report()[0]["size_class"] == 4
    for shape in ((64, 64), (5, 4), (256, 128)):
        assert not any(dense(wc.slide(*shape, np.uint16), INT | GLCM)), shape
    assert not any(dense(wc.slide(257, 33, np.uint32, "range4m"), INT | GLCM))
    assert dense(wc.slide(257, 33, np.uint32, "range70000"), INT | GLCM) == [True]
    for extra in (_abi.FAM_GLRLM, _abi.FAM_GABOR, _abi.FAM_NGLDM):
        assert not any(dense(wc.slide(257, 33, np.uint16), INT | GLCM | extra)), extra
    # a stack of three: the middle slide's range is beyond the histogram workspace -- the last launch group is the third slide's, dense
    stack = np.stack([wc.slide(257, 33, np.uint32, "random"), wc.slide(257, 33, np.uint32, "range4m"), wc.slide(257, 33, np.uint32, "zeros")])
    assert dense(stack, INT | GLCM) == [True] and hip_ctx.launch_report()[0]["rois"] == 1
    _invariant(hip_ctx, list(stack), INT | GLCM, s, "mixed stack")


def test_every_served_family_through_the_cloud_route(hip_ctx):
    s = wc.settings("gd64")
    for w, h in ((96, 70), (257, 33)):
        for dt in wc.DTYPES:
            _invariant(hip_ctx, [wc.slide(w, h, dt, "zeros")], _abi.FAM_WHOLE_SLIDE, s, (w, h, np.dtype(dt).name, "all ten"))
    img = wc.slide(96, 70, np.uint16, "zeros")
    for bit in range(2, 10):
        _invariant(hip_ctx, [img], 1 << bit, s, ("bit", bit))
        _invariant(hip_ctx, [img], (1 << bit) | INT | GLCM, s, ("bit and the dense pair", bit))


def test_stacks_chunks_and_device_memory(hip_ctx):
    import torch
    s = wc.settings("gd64")
    mask = INT | GLCM
    imgs = [wc.slide(300, 200, np.uint16, "zeros" if k == 3 else "random", seed=k) for k in range(5)]
    stack = np.stack(imgs)
    alone = np.vstack([hip_ctx.featurize_slides_host(i[None], mask, s) for i in imgs])
    _assert_same(alone, hip_ctx.featurize_host(wc.slide_batch(imgs), mask, s), "each slide alone")
    whole = hip_ctx.featurize_slides_host(stack, mask, s)
    _assert_same(whole, alone, "one call")
    # 2 MiB: a slide takes 8 B per pixel of cloud and two staging copies of its 120000 bytes -- two slides fit, three do not
    chunked = hip_ctx.featurize_slides_host(stack, mask, s, max_device_bytes=2 << 20)
    _assert_same(chunked, alone, "chunks")
    assert hip_ctx.launch_report()[-1]["rois"] == 1                      # three chunks (2 + 2 + 1): the last launch group held the fifth slide alone
    with pytest.raises(_lib.NyxHipError) as ei:
        hip_ctx.featurize_slides_host(stack, mask, s, max_device_bytes=1 << 16)
    assert ei.value.code == 5
    assert hip_ctx.featurize_slides_host(stack[:0], mask, s).shape == (0, hip_ctx.n_columns(mask, s))
    # device memory in and out
    ncol = hip_ctx.n_columns(mask, s)
    for dt, tdt in ((np.uint8, torch.uint8), (np.uint16, torch.int16), (np.uint32, torch.int32)):
        st = np.stack([wc.slide(259, 127, dt, seed=k) for k in range(3)])
        d_in = torch.from_numpy(st.view(np.int16) if dt == np.uint16 else st.view(np.int32) if dt == np.uint32 else st).to("cuda:0")
        d_out = torch.full((3, ncol + 2), -1.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        hip_ctx.featurize_slides_device(d_in.data_ptr(), np.dtype(dt).itemsize, 3, 127, 259, mask, s, d_out.data_ptr(), ncol + 2)
        out = d_out.cpu().numpy()
        _assert_same(out[:, :ncol], hip_ctx.featurize_slides_host(st, mask, s), ("device", np.dtype(dt).name))
        assert (out[:, ncol:] == -1.0).all()
        # ... and from the middle of the device array: a chunk base that is not 16-byte aligned for the 8-bit stack
        hip_ctx.featurize_slides_device(d_in.data_ptr() + 127 * 259 * np.dtype(dt).itemsize, np.dtype(dt).itemsize, 2, 127, 259, mask, s, d_out.data_ptr(), ncol + 2)
        _assert_same(d_out.cpu().numpy()[:2, :ncol], out[1:, :ncol], ("device, offset base", np.dtype(dt).name))


def test_refusals(hip_ctx):
    s = wc.settings("gd64")
    img = wc.slide(16, 16, np.uint16)[None]
    for fam in (_abi.FAM_SMOMS, _abi.FAM_IMOMS, _abi.FAM_RADIAL, _abi.FAM_CIRCLES, _abi.FAM_SMOMS | INT):
        with pytest.raises(_lib.NyxHipError, match="whole-slide mode") as ei:
            hip_ctx.featurize_slides_host(img, fam, s)
        assert ei.value.code == 4
    for bit in (12, 14, 26, 27, 28, 29, 30, 31):
        with pytest.raises(_lib.NyxHipError) as ei:
            hip_ctx.featurize_slides_host(img, (1 << bit) | INT, s)
        assert ei.value.code == 1
    # only the header is validated: nothing of that size exists
    import ctypes as C
    lib = _lib.load()
    out = np.zeros(64)
    for w, h in ((65535, 1), (1, 65535), (0, 4), (4, 0)):
        t = _abi.Tiles()
        t.inten = img.ctypes.data; t.inten_dtype = _abi.U16; t.width = w; t.height = h; t.n_tiles = 1; t.memory = _abi.MEM_HOST
        assert lib.nyxhip_featurize_slides(hip_ctx._h, C.byref(t), INT, C.byref(s), out.ctypes.data, 64) == 4
        assert b"whole-slide mode" in lib.nyxhip_last_error(hip_ctx._h)
    t = _abi.Tiles()
    t.inten = img.ctypes.data; t.label = img.ctypes.data; t.inten_dtype = _abi.U16; t.width = 16; t.height = 16; t.n_tiles = 1
    assert lib.nyxhip_featurize_slides(hip_ctx._h, C.byref(t), INT, C.byref(s), out.ctypes.data, 64) == 1
    t.label = None
    assert lib.nyxhip_featurize_slides(hip_ctx._h, C.byref(t), INT, C.byref(s), out.ctypes.data, 8) == 1     # out_ld below the column count
    assert (out == 0).all()


def test_through_the_nyxus_class(tmp_path):
    d = tmp_path / "int"
    d.mkdir()
    imgs = {"b_first.tif": wc.slide(257, 33, np.uint16, "zeros", seed=1), "c_second.tif": wc.slide(300, 200, np.uint8, "random", seed=2),
            "a_third.tif": wc.slide(257, 33, np.uint16, "random", seed=3)}
    for name, a in imgs.items():
        synth.write_tiled_tiff(str(d / name), a, tile=128)
    feats = ["*ALL_INTENSITY*", "*ALL_GLCM*"]
    nyx = nyxus_amd.Nyxus(feats)
    paths = [str(d / n) for n in imgs]
    df = nyx.featurize_files(paths, None, True)
    assert len(df) == 3 and list(df["intensity_image"]) == paths and (df["mask_image"] == "").all()
    assert (df["ROI_label"] == 1).all() and df["ROI_label"].dtype == np.uint32 and (df["t_index"] == 0).all()
    mask, s = INT | GLCM, _abi.default_settings(64)
    names = _lib.column_names(mask, s)
    assert list(df.columns[4:]) == names
    b = wc.slide_batch(list(imgs.values()))
    want = po.oracle_featurize(b, mask, s)
    _lib.load().nyxhip_finalize_table(want.ctypes.data, want.shape[0], want.shape[1], want.shape[1], s.soft_nan)
    bad = parity.compare_tables(np.ascontiguousarray(df[names].values, dtype=np.float64), want, names, batch=b)
    assert not bad, bad[:8]
    order = sorted(range(3), key=lambda k: list(imgs)[k])
    for call in (lambda: nyx.featurize_directory(str(d)), lambda: nyx.featurize_directory(str(d), str(d)),
                 lambda: nyxus_amd.Nyxus(feats).featurize_directory(str(d), file_pattern=r".*\.tif")):
        dd = call()
        assert list(dd["intensity_image"]) == [os.path.join(str(d), n) for n in sorted(imgs)]
        assert (dd["mask_image"] == "").all() and (dd["ROI_label"] == 1).all()
        _assert_same(np.ascontiguousarray(dd[names].values, dtype=np.float64), np.ascontiguousarray(df[names].values[order], dtype=np.float64), "directory")
    assert nyx.featurize_files(paths, ["ignored"], True).equals(df)
