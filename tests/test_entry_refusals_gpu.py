"""What the batch and tile entries refuse, and in which words: one refused call per row of a table, each call with exactly one fault.

Every row names an entry, spoils one argument of an otherwise valid call (the unspoiled calls pass: the last test) and states the return
code and a distinctive part of nyxhip_last_error as the entry's source gives them.  The batch is two ROIs of 3 x 3 pixels, the stack one
8 x 8 tile with the same two boxes; no kernel needs to run for a refusal, and the caller's table stays untouched."""
import ctypes as C

import numpy as np
import pytest

from nyxus_amd import _abi, _lib

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED, ROI_TOO_LARGE = 1, 4, 5
FAMILY_MASK = _abi.FAM_INTENSITY | _abi.FAM_GLCM


def two_boxes() -> _abi.HostBatch:
    rois = [dict(label=k + 1, x=np.repeat(np.arange(3), 3) + 4 * k, y=np.tile(np.arange(3), 3) + 4 * k, inten=np.arange(1, 10, dtype=np.uint32) + k)
            for k in range(2)]
    b = _abi.batch_from_rois(rois)
    b.image_offset = np.array([0, 2], np.uint64)
    return b


class Args:
    """Every argument of a call, all of them valid; a row of the table spoils exactly one."""

    def __init__(self):
        self.hb = two_boxes()
        self.b = self.hb.c_struct()
        self.s = _abi.default_settings(64)
        self.ox, self.oy = self.hb.origin_x.ctypes.data, self.hb.origin_y.ctypes.data
        self.io, self.n_images = self.hb.image_offset.ctypes.data, 1
        self.distance, self.mmask, self.mask = 5, _abi.MORPH_ALL, FAMILY_MASK
        self.table = np.full((2, 256), -7.0)
        self.out = self.table.ctypes.data
        self.ld_delta = 0                                # out_ld = the entry's column count + ld_delta
        self.lab = np.zeros((1, 8, 8), np.uint32)
        self.lab[0, :3, :3] = 1; self.lab[0, 4:7, 4:7] = 2
        self.inten = np.arange(1, 65, dtype=np.uint32).reshape(1, 8, 8)
        t = self.t = _abi.Tiles()
        t.inten = self.inten.ctypes.data; t.label = self.lab.ctypes.data
        t.inten_dtype = t.label_dtype = _abi.U32
        t.width = t.height = 8; t.n_tiles = 1; t.memory = _abi.MEM_HOST; t.slide_mode = _abi.SLIDE_MONTAGE
        self.n = C.c_uint64(0)
        self.n_out = C.byref(self.n)


def p(x):
    return C.byref(x) if x is not None else None


# entry -> (column count, call).  The tile calls keep their rows in the context (NULL outputs), as the Python wrappers do.
BATCH = {
    "featurize_batch_at": (lambda L, a: L.nyxhip_n_columns(a.mask, C.byref(a.s)),
                           lambda L, h, a, ld: L.nyxhip_featurize_batch_at(h, p(a.b), a.ox, a.oy, a.mask, p(a.s), a.out, ld)),
    "ih_batch": (lambda L, a: _abi.IH_COLS, lambda L, h, a, ld: L.nyxhip_ih_batch(h, p(a.b), p(a.s), a.out, ld)),
    "imq_batch": (lambda L, a: _abi.IMQ_COLS, lambda L, h, a, ld: L.nyxhip_imq_batch(h, p(a.b), p(a.s), a.out, ld)),
    "morph_batch": (lambda L, a: L.nyxhip_morph_n_columns(_abi.MORPH_ALL),
                    lambda L, h, a, ld: L.nyxhip_morph_batch(h, p(a.b), a.ox, a.oy, a.mmask, p(a.s), a.out, ld)),
    "neighbors_batch": (lambda L, a: _abi.NEIGHBOR_COLS,
                        lambda L, h, a, ld: L.nyxhip_neighbors_batch(h, p(a.b), a.ox, a.oy, a.io, a.n_images, a.distance, p(a.s), a.out, ld)),
    "hexpoly_batch": (lambda L, a: _abi.HEXPOLY_COLS,
                      lambda L, h, a, ld: L.nyxhip_hexpoly_batch(h, p(a.b), a.ox, a.oy, a.io, a.n_images, a.distance, p(a.s), a.out, ld)),
}
TILES = {
    "featurize_tiles_v2": (lambda L, a: L.nyxhip_n_columns(a.mask, C.byref(a.s)),
                           lambda L, h, a, ld: L.nyxhip_featurize_tiles_v2(h, p(a.t), a.mask, p(a.s), None, None, 0, None, 0, a.n_out)),
    "neighbors_tiles": (lambda L, a: _abi.NEIGHBOR_COLS,
                        lambda L, h, a, ld: L.nyxhip_neighbors_tiles(h, p(a.t), a.distance, p(a.s), None, None, 0, None, 0, a.n_out)),
    "ih_tiles": (lambda L, a: _abi.IH_COLS, lambda L, h, a, ld: L.nyxhip_ih_tiles(h, p(a.t), p(a.s), None, None, 0, None, 0, a.n_out)),
    "imq_tiles": (lambda L, a: _abi.IMQ_COLS, lambda L, h, a, ld: L.nyxhip_imq_tiles(h, p(a.t), p(a.s), None, None, 0, None, 0, a.n_out)),
    "morph_tiles": (lambda L, a: L.nyxhip_morph_n_columns(_abi.MORPH_ALL),
                    lambda L, h, a, ld: L.nyxhip_morph_tiles(h, p(a.t), a.mmask, p(a.s), None, None, 0, None, 0, a.n_out)),
    "hexpoly_tiles": (lambda L, a: _abi.HEXPOLY_COLS,
                      lambda L, h, a, ld: L.nyxhip_hexpoly_tiles(h, p(a.t), a.distance, p(a.s), None, None, 0, None, 0, a.n_out)),
}
ENTRIES = {**BATCH, **TILES}

# the array a row takes away, and what the entry says then
NULL_ARRAY = {
    "featurize_batch_at": ("inten", "batch has null array pointers"),
    "ih_batch": ("inten", "the intensity-histogram entries read px_offset, inten, min_inten, max_inten"),
    "imq_batch": ("bbox_w", "the image-quality entries read px_offset, x, y, inten, bbox_w, bbox_h, min_inten, max_inten"),
    "morph_batch": ("x", "batch has null array pointers"),
    "neighbors_batch": ("roi_label", "the neighbor entries read roi_label"),
    "hexpoly_batch": ("roi_label", "the neighbor entries read roi_label"),
}
TAKES_ORIGINS = ("featurize_batch_at", "morph_batch", "neighbors_batch", "hexpoly_batch")
TAKES_IMAGES = ("neighbors_batch", "hexpoly_batch")
TAKES_DISTANCE = ("neighbors_batch", "hexpoly_batch", "neighbors_tiles", "hexpoly_tiles")


def put(obj, **fields):
    def spoil(a):
        for k, v in fields.items():
            setattr(getattr(a, obj) if obj else a, k, v)
    return spoil


def descending_offsets(a):
    a.hb.px_offset[:] = [0, 9, 5]


def wide_box(a):
    a.hb.bbox_w[0] = 65536


def short_images(a):
    a.keep = np.array([0, 1], np.uint64)
    a.io = a.keep.ctypes.data


def rows():
    out = []
    for e in BATCH:
        out += [
            (e, "null settings", put(None, s=None), INVALID_ARG, "null batch / settings / out_table"),
            (e, "null out", put(None, out=None), INVALID_ARG, "null batch / settings / out_table"),
            (e, "null " + NULL_ARRAY[e][0], put("b", **{NULL_ARRAY[e][0]: None}), INVALID_ARG, NULL_ARRAY[e][1]),
            (e, "ld one short", put(None, ld_delta=-1), INVALID_ARG, "out_ld smaller than the column count"),
            (e, "memory 99", put("b", memory=99), INVALID_ARG, "bad batch->memory"),
            (e, "descending px_offset", descending_offsets, INVALID_ARG, "px_offset is not monotone"),
        ]
    for e in TAKES_ORIGINS:
        out.append((e, "origin_x alone", put(None, oy=None), INVALID_ARG, "origin_x and origin_y must both be given or both NULL"))
    for e in TAKES_IMAGES:
        out.append((e, "image_offset of no image", put(None, n_images=0), INVALID_ARG, "image_offset given with n_images == 0"))
        out.append((e, "image_offset ends early", short_images, INVALID_ARG, "image_offset must run from 0 to n_roi"))
    for e in ("morph_batch", "morph_tiles"):
        out.append((e, "morphology mask 0x10", put(None, mmask=0x10), INVALID_ARG, "bad morphology mask"))
    for e in TAKES_DISTANCE:
        out.append((e, "distance 0", put(None, distance=0), INVALID_ARG, "pixel_distance must be greater than zero"))
        out.append((e, "distance 46341", put(None, distance=46341), UNSUPPORTED, "pixel_distance beyond 46340"))
    for e in ("ih_batch", "ih_tiles"):
        out.append((e, "4097 bins under ibsi", put("s", grey_depth=4097, ibsi=1), UNSUPPORTED, "grey_depth beyond 4096 bins"))
    out.append(("imq_batch", "box side 65536", wide_box, ROI_TOO_LARGE, "wider or taller than 65535 pixels"))
    for e in TILES:
        out += [
            (e, "no tile", put("t", n_tiles=0), INVALID_ARG, "n_tiles must be >= 1"),
            (e, "element type 3", put("t", inten_dtype=3), INVALID_ARG, "tile element types must be NYXHIP_U8 / U16 / U32"),
            (e, "slide_mode 7", put("t", slide_mode=7), INVALID_ARG, "bad slide_mode"),
            (e, "null n_roi_out", put(None, n_out=None), INVALID_ARG, "null tiles / settings / n_roi_out"),
        ]
    return out


ROWS = rows()


@pytest.mark.parametrize("row", ROWS, ids=[f"{r[0]}-{r[1].replace(' ', '_')}" for r in ROWS])
def test_one_fault_is_refused_with_its_code_and_words(hip_ctx, row):
    entry, fault, spoil, code, words = row
    L = _lib.load()
    a = Args()
    n_cols, call = ENTRIES[entry]
    ld = n_cols(L, a)
    spoil(a)
    rc = call(L, hip_ctx._h, a, ld + a.ld_delta)
    said = (L.nyxhip_last_error(hip_ctx._h) or b"").decode()
    print(f"{entry}, {fault}: code {rc}, '{said}'")
    assert rc == code and words in said, (entry, fault, rc, said)
    assert (a.table == -7.0).all() and a.n.value == 0


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_the_unspoiled_call_passes(hip_ctx, entry):
    L = _lib.load()
    a = Args()
    n_cols, call = ENTRIES[entry]
    ld = n_cols(L, a)
    assert call(L, hip_ctx._h, a, ld) == 0, (L.nyxhip_last_error(hip_ctx._h) or b"").decode()
    if entry in TILES:
        labels, tiles = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
        assert a.n.value == 2 and L.nyxhip_fetch_result(hip_ctx._h, labels.ctypes.data, tiles.ctypes.data, a.out, ld) == 0
        assert labels.tolist() == [1, 2]
    rows = a.table.ravel()                                                   # two rows at out_ld = the column count, nothing behind them
    assert (rows[:2 * ld].reshape(2, ld) != -7.0).any(axis=1).all() and (rows[2 * ld:] == -7.0).all()
