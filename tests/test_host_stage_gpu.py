"""A batch gives the same table from host memory and from device memory, through every batch entry, and a context keeps nothing of a call.

The six batch entries (the family entry, IH, image quality, morphology, neighbors, hexagonality / polygonality) stage a host batch into one
device slab and run the device function that a device batch reaches directly.  The same batch goes through NYXHIP_MEM_HOST and through
NYXHIP_MEM_DEVICE (torch tensors; the extrema fields left 0, and once more stated), and the tables are compared on their raw 64-bit
patterns, NaN included.  The batch is 4 ROIs in boxes of up to 8 x 8, one of them without a pixel; the variants are with and without
origins, with an image_offset of two images and with none, a batch of empty ROIs only (no pixel to upload), n_roi == 0, and a table wider
than its columns whose padding stays untouched.  The last test calls the batch and tile entries back to back on one context and compares
every table with the one the same call gave on a context of its own."""
import ctypes as C

import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from tests import neighbors_cases as nc, synth
from tests.radial_cases import disc

pytestmark = pytest.mark.gpu

ENTRIES = ("family", "ih", "imq", "morph", "neighbors", "hexpoly")
TAKES_ORIGINS = ("family", "morph", "neighbors", "hexpoly")
TAKES_IMAGES = ("neighbors", "hexpoly")
FAMILY_MASK = _abi.FAM_INTENSITY | _abi.FAM_FERET            # FERET reads the origins
DISTANCE = 5
PAD = -7.0
_HOST = {}


def settings():
    return _abi.default_settings(64)


def label_images():
    """Two 16 x 24 images: a disc in a 7 x 7 box, a full 8 x 8 box and a 1 x 3 bar | the same geometry under other labels."""
    lab = np.zeros((16, 24), np.uint32)
    nc.put(lab, disc(3), 1, 1, 1)
    nc.put(lab, np.ones((8, 8), bool), 7, 10, 3)
    nc.put(lab, np.ones((1, 3), bool), 2, 12, 4)
    return [lab, np.where(lab > 0, lab + 10, 0).astype(np.uint32)]


def with_empty_roi(b: _abi.HostBatch, at: int, label: int) -> _abi.HostBatch:
    """The batch with an ROI of no pixel (an empty box at (5, 5)) put in front of row `at`."""
    ins = lambda a, v: np.insert(np.asarray(a), at, v)
    return _abi.HostBatch(ins(b.roi_label, label), ins(b.px_offset, b.px_offset[at]), b.x, b.y, b.inten, ins(b.bbox_w, 0), ins(b.bbox_h, 0),
                          ins(b.min_inten, 0), ins(b.max_inten, 0), origin_x=ins(b.origin_x, 5), origin_y=ins(b.origin_y, 5))


def mixed_batch() -> _abi.HostBatch:
    """Labels 1, 2 (empty), 3, 4; as two images: rows [0, 2) and [2, 4)."""
    lab = label_images()[0]
    b = with_empty_roi(_abi.batch_from_rois(synth.rois_from_tile(nc.intensity(lab, 7), lab)), 1, 2)
    assert b.n_roi == 4 and np.diff(b.px_offset.astype(np.int64)).tolist() == [29, 0, 64, 3] and int(max(b.bbox_w.max(), b.bbox_h.max())) == 8
    return b


def empty_batch() -> _abi.HostBatch:
    z = np.zeros(4, np.uint32)
    none = np.zeros(0, np.uint32)
    return _abi.HostBatch(np.arange(1, 5), np.zeros(5, np.uint64), none, none, none, z, z, z, z, origin_x=z + 3, origin_y=z + 9)


def n_cols(entry):
    L = _lib.load()
    return {"family": L.nyxhip_n_columns(FAMILY_MASK, C.byref(settings())), "ih": _abi.IH_COLS, "imq": _abi.IMQ_COLS,
            "morph": L.nyxhip_morph_n_columns(_abi.MORPH_ALL), "neighbors": _abi.NEIGHBOR_COLS, "hexpoly": _abi.HEXPOLY_COLS}[entry]


def call(ctx, entry, cb, ox, oy, io, n_images, out, ld):
    """The entry on a nyxhip_batch and raw pointers (host or device alike); returns the code."""
    L, h, s = _lib.load(), ctx._h, settings()
    if entry == "family":
        return L.nyxhip_featurize_batch_at(h, C.byref(cb), ox, oy, FAMILY_MASK, C.byref(s), out, ld)
    if entry == "ih":
        return L.nyxhip_ih_batch(h, C.byref(cb), C.byref(s), out, ld)
    if entry == "imq":
        return L.nyxhip_imq_batch(h, C.byref(cb), C.byref(s), out, ld)
    if entry == "morph":
        return L.nyxhip_morph_batch(h, C.byref(cb), ox, oy, _abi.MORPH_ALL, C.byref(s), out, ld)
    f = L.nyxhip_neighbors_batch if entry == "neighbors" else L.nyxhip_hexpoly_batch
    return f(h, C.byref(cb), ox, oy, io, n_images, DISTANCE, C.byref(s), out, ld)


def said(ctx):
    return (_lib.load().nyxhip_last_error(ctx._h) or b"").decode()


def images_of(b, images):
    return np.array([0, 2, b.n_roi], np.uint64) if images else None


def host_table(ctx, entry, b, origins, images, extra=0):
    nc_, io = n_cols(entry), images_of(b, images)
    T = np.full((b.n_roi, nc_ + extra), PAD)
    rc = call(ctx, entry, b.c_struct(), b.origin_x.ctypes.data if origins else None, b.origin_y.ctypes.data if origins else None,
              io.ctypes.data if images else None, 2 if images else 0, T.ctypes.data, nc_ + extra)
    assert rc == 0, (entry, said(ctx))
    assert (T[:, nc_:] == PAD).all(), entry                                  # nothing is written beyond the entry's columns
    return np.ascontiguousarray(T[:, :nc_])


def device_table(ctx, entry, b, origins, images, stated, extra=0):
    import torch
    dev = torch.device("cuda", 0)
    view = {2: np.int16, 4: np.int32, 8: np.int64}

    def up(a):                                                               # (a tensor of no element has no address: one spare element)
        a = np.ascontiguousarray(a)
        a = np.concatenate([a, np.zeros(1, a.dtype)])
        return torch.from_numpy(a.view(view[a.dtype.itemsize])).to(dev)
    keep = {k: up(getattr(b, k)) for k in ("roi_label", "px_offset", "x", "y", "inten", "bbox_w", "bbox_h", "min_inten", "max_inten")}
    ox, oy = (up(b.origin_x), up(b.origin_y)) if origins else (None, None)
    io = up(images_of(b, images)) if images else None
    cb = _abi.Batch()
    cb.n_roi = b.n_roi
    for k, t in keep.items():
        setattr(cb, k, t.data_ptr())
    cb.memory = _abi.MEM_DEVICE
    if stated:
        h = b.c_struct()
        cb.max_px, cb.max_bbox_area, cb.max_inten_range, cb.max_bbox_side = h.max_px, h.max_bbox_area, h.max_inten_range, h.max_bbox_side
    nc_ = n_cols(entry)
    out = torch.full((b.n_roi, nc_ + extra), PAD, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rc = call(ctx, entry, cb, ox.data_ptr() if origins else None, oy.data_ptr() if origins else None, io.data_ptr() if images else None,
              2 if images else 0, out.data_ptr(), nc_ + extra)
    assert rc == 0, (entry, said(ctx))
    T = out.cpu().numpy()
    assert (T[:, nc_:] == PAD).all(), entry
    return np.ascontiguousarray(T[:, :nc_])


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)).all()


def variants(entry):
    return [(o, i) for o in ((True, False) if entry in TAKES_ORIGINS else (False,)) for i in ((True, False) if entry in TAKES_IMAGES else (False,))]


def host_rows(ctx, entry, origins, images):
    """The mixed batch through the host form of an entry, computed once and shared."""
    key = (entry, origins, images)
    if key not in _HOST:
        _HOST[key] = host_table(ctx, entry, mixed_batch(), origins, images)
    return _HOST[key]


@pytest.mark.parametrize("entry", ENTRIES)
def test_host_and_device_batches_give_the_same_bits(hip_ctx, entry):
    b = mixed_batch()
    for origins, images in variants(entry):
        host = host_rows(hip_ctx, entry, origins, images)
        assert host.shape == (4, n_cols(entry))
        for stated in (False, True):
            assert same_bits(device_table(hip_ctx, entry, b, origins, images, stated), host), (entry, origins, images, stated)
        assert same_bits(host_table(hip_ctx, entry, b, origins, images), host), (entry, origins, images)       # and again from the host


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_wider_table_keeps_its_padding(hip_ctx, entry):
    b = mixed_batch()
    origins, images = variants(entry)[0]
    host = host_rows(hip_ctx, entry, origins, images)
    assert same_bits(host_table(hip_ctx, entry, b, origins, images, extra=3), host)
    assert same_bits(device_table(hip_ctx, entry, b, origins, images, False, extra=3), host)


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_batch_of_empty_rois_uploads_no_pixel(hip_ctx, entry):
    b = empty_batch()
    for origins, images in variants(entry):
        host = host_table(hip_ctx, entry, b, origins, images)
        assert same_bits(device_table(hip_ctx, entry, b, origins, images, False), host), (entry, origins, images)
    assert same_bits(host_rows(hip_ctx, entry, *variants(entry)[0]), host_table(hip_ctx, entry, mixed_batch(), *variants(entry)[0]))


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_roi_is_no_work(hip_ctx, entry):
    T = np.full(n_cols(entry), PAD)
    for memory in (_abi.MEM_HOST, _abi.MEM_DEVICE):
        cb = _abi.Batch()
        cb.n_roi = 0; cb.memory = memory
        assert call(hip_ctx, entry, cb, None, None, None, 0, T.ctypes.data, n_cols(entry)) == 0, (entry, memory, said(hip_ctx))
    assert (T == PAD).all()


def test_a_context_keeps_nothing_of_a_call(hip_ctx):
    """The batch and tile entries back to back on one context, interleaved, forwards and backwards: every table has the bits the same call
    gave on a context of its own (the staging slab, the kept result and its column count, the window source are per call)."""
    s = settings()
    b = mixed_batch()
    b.image_offset = images_of(b, True)
    M = np.stack(label_images())
    I = np.stack([nc.intensity(m, 7 + k) for k, m in enumerate(M)])
    window_mask = _abi.FAM_INTENSITY | _abi.FAM_GLCM                         # the tile path reads these two from the tiles' windows
    calls = [
        ("family batch", lambda c: c.featurize_host(b, FAMILY_MASK, s)),
        ("ih tiles", lambda c: c.ih_tiles_host(I, M, s)[2]),
        ("ih batch", lambda c: c.ih_host(b, s)),
        ("hexpoly tiles", lambda c: c.hexpoly_tiles_host(I, M, DISTANCE, s)[2]),
        ("imq batch", lambda c: c.imq_host(b, s)),
        ("family tiles", lambda c: c.featurize_tiles_host(I, M, window_mask, s)[2]),
        ("morph batch", lambda c: c.morph_host(b, _abi.MORPH_ALL, s)),
        ("neighbors tiles", lambda c: c.neighbors_tiles_host(I, M, DISTANCE, s)[2]),
        ("neighbors batch", lambda c: c.neighbors_host(b, DISTANCE, s)),
        ("morph tiles", lambda c: c.morph_tiles_host(I, M, _abi.MORPH_ALL, s)[2]),
        ("hexpoly batch", lambda c: c.hexpoly_host(b, DISTANCE, s)),
        ("imq tiles", lambda c: c.imq_tiles_host(I, M, s)[2]),
    ]
    alone = {}
    for name, f in calls:
        own = _lib.Context(0)
        try:
            alone[name] = f(own)
        finally:
            own.close()
        assert alone[name].shape[0] == (4 if name.endswith("batch") else 6), name
    for name, f in calls + calls[::-1]:
        assert same_bits(f(hip_ctx), alone[name]), name
