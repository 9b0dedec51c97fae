"""The device label scan for volumes on the GPU (nyxhip_assemble_volumes; `assembly="device"` of Nyxus3D.featurize): every array of the
assembled batch, its volume indices, stated extrema and row count against the host assembly (clouds_from_volume + batch3d_from_rois),
bit for bit, on the cases of tests/volscan_cases.py; the life of the batch on its context; the assembled batch through each of the five
volume entries against the host batch through the same entry; the two routes of Nyxus3DShape.featurize; every refusal."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from nyxus_amd.nyxus3d import Nyxus3DShape
from tests import volscan_cases as vc

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED, ROI_TOO_LARGE = 1, 4, 5
ARRAYS = ("roi_label", "px_offset", "x", "y", "z", "inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@lru_cache(maxsize=None)
def case(name):
    I, L = vc.ENTRY_CASES[name[6:]]() if name.startswith("entry:") else vc.CASES[name]()
    b, vol = vc.host_assembly(I, L)
    for a in (I, L, vol, *(getattr(b, k) for k in ARRAYS)):
        a.setflags(write=False)                              # shared among the tests: computed once, never changed
    return I, L, b, vol


def fetch(ptr, n, dtype):
    """n elements of device memory at `ptr` (through the HIP runtime the library is linked with)."""
    out = np.empty(n, dtype)
    if n:
        assert ptr
        memcpy = _lib.load().hipMemcpy
        memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        memcpy.restype = C.c_int
        assert memcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


def device_arrays(a):
    """Every array of the assembled batch and its volume indices, copied back."""
    cb, n = a.batch, a.n_roi
    off = fetch(cb.px_offset, n + 1 if n else 0, np.uint64)
    npx = int(off[-1]) if n else 0
    got = {"px_offset": off if n else np.zeros(1, np.uint64), "roi_label": fetch(cb.roi_label, n, np.uint32)}
    for k in ("x", "y", "z"):
        got[k] = fetch(getattr(cb, k), npx, np.uint16)
    got["inten"] = fetch(cb.inten, npx, np.uint32)
    for k in ("bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten"):
        got[k] = fetch(getattr(cb, k), n, np.uint32)
    got["volume_index"] = fetch(a.volume_index_ptr, n, np.uint32)
    return got


def check_assembled(a, b, vol, max_device_bytes=0, what=""):
    cb = a.batch
    assert a.n_roi == cb.n_roi == b.n_roi, what
    assert cb.memory == _abi.MEM_DEVICE and cb.slide_min is None and cb.slide_max is None and cb.max_device_bytes == max_device_bytes, what
    got = device_arrays(a)
    for k in ARRAYS:
        want = getattr(b, k)
        assert got[k].dtype == want.dtype and got[k].shape == want.shape and (got[k] == want).all(), (what, k, got[k][:16], want[:16])
    assert (got["volume_index"] == vol).all(), what
    # nyxhip_assembled_rows agrees with the device arrays
    assert (a.labels == got["roi_label"]).all() and (a.volume_index == got["volume_index"]).all(), what
    h = b.c_struct(stated=True)
    assert (cb.max_px, cb.max_bbox_cells, cb.max_inten_range) == (h.max_px, h.max_bbox_cells, h.max_inten_range), what


@pytest.mark.parametrize("name", list(vc.CASES))
def test_host_volumes_equal_the_host_assembly(ctx, name):
    I, L, b, vol = case(name)
    check_assembled(ctx.assemble_volumes_host(I, L), b, vol, what=name)


def test_confetti_on_a_fresh_context_grows_its_tables():
    """8000 labels from the first table size (4096 slots): the scan overflows, the tables grow, the chunk is scanned again."""
    I, L, b, vol = case("confetti")
    c = _lib.Context(0)
    try:
        check_assembled(c.assemble_volumes_host(I, L), b, vol, what="confetti, fresh context")
        check_assembled(c.assemble_volumes_host(I, L), b, vol, what="confetti, the table size that served the last call")
    finally:
        c.close()


def to_device(a):
    import torch
    view = {1: np.uint8, 2: np.int16, 4: np.int32}[a.dtype.itemsize]
    return torch.from_numpy(np.array(a).view(view)).to(torch.device("cuda", 0))


@pytest.mark.parametrize("name", ["stack_three", "seam_w257", "seam_h_plus", "checkerboard", "confetti", "slab_box", "no_label"])
def test_device_volumes_equal_the_host_assembly(ctx, name):
    import torch
    I, L, b, vol = case(name)
    ti, tl = to_device(I), to_device(L)
    torch.cuda.synchronize()
    a = ctx.assemble_volumes_device(ti.data_ptr(), _abi.volume_dtype(I.dtype), tl.data_ptr(), _abi.volume_dtype(L.dtype), I.shape)
    check_assembled(a, b, vol, what=name)


@pytest.mark.parametrize("dl", vc.DTYPES, ids=lambda d: "label_" + np.dtype(d).name)
@pytest.mark.parametrize("di", vc.DTYPES, ids=lambda d: "inten_" + np.dtype(d).name)
@pytest.mark.parametrize("memory", ["host", "device"])
def test_every_dtype_pair(ctx, memory, di, dl):
    import torch
    I, L = vc.small_types(di, dl)
    b, vol = vc.host_assembly(I, L)
    if memory == "host":
        a = ctx.assemble_volumes_host(I, L)
    else:
        ti, tl = to_device(I), to_device(L)
        torch.cuda.synchronize()
        a = ctx.assemble_volumes_device(ti.data_ptr(), _abi.volume_dtype(di), tl.data_ptr(), _abi.volume_dtype(dl), I.shape)
    check_assembled(a, b, vol, what=(memory, di, dl))


def test_budget_chunks_and_refusal():
    """One and a half volumes of budget: a three-volume host stack goes in three chunks (fresh context: the first table size).  One byte
    less than a volume and its table: refused; the context serves the next call."""
    I, L, b, vol = case("stack_three")
    per = vc.chunk_bytes(I.shape[1:], I.dtype, L.dtype)
    c = _lib.Context(0)
    try:
        check_assembled(c.assemble_volumes_host(I, L, max_device_bytes=per + per // 2), b, vol, per + per // 2, "three chunks")
        check_assembled(c.assemble_volumes_host(I, L, max_device_bytes=2 * per), b, vol, 2 * per, "two chunks")
        with pytest.raises(_lib.NyxHipError) as ei:
            c.assemble_volumes_host(I, L, max_device_bytes=per - 1)
        assert ei.value.code == ROI_TOO_LARGE
        check_assembled(c.assemble_volumes_host(I, L), b, vol, what="after the refusal")
    finally:
        c.close()


def test_chunks_of_a_stack_with_slab_boxes_and_confetti():
    """Chunks whose rows take the slab form of the cloud launch, and chunks whose tables grow: a stack of the slab case twice and of the
    confetti case twice, a chunk per volume."""
    for name in ("slab_box", "confetti"):
        I1, L1, _, _ = case(name)
        I, L = np.concatenate([I1, I1[:, ::-1]]), np.concatenate([L1, L1[:, ::-1]])
        b, vol = vc.host_assembly(I, L)
        budget = vc.chunk_bytes(I.shape[1:], I.dtype, L.dtype) + 4096
        if name == "confetti":                               # both volumes fit with their first tables, one with the table it grows to
            budget += 4 * vc.TABLE_WORDS * (4 * vc.CAP_FIRST - vc.CAP_FIRST)
            assert 2 * vc.chunk_bytes(I.shape[1:], I.dtype, L.dtype) <= budget < 2 * (budget - 4096)
        c = _lib.Context(0)
        try:
            check_assembled(c.assemble_volumes_host(I, L, max_device_bytes=budget), b, vol, budget, name + ", a chunk per volume")
        finally:
            c.close()


def test_batch_life_on_its_context(ctx):
    I1, L1, b1, vol1 = case("checkerboard")
    I2, L2, b2, vol2 = case("shell")
    a1 = ctx.assemble_volumes_host(I1, L1)
    a2 = ctx.assemble_volumes_host(I2, L2)                   # replaces the first
    check_assembled(a2, b2, vol2, what="second assemble")
    lib = _lib.load()
    lab = np.zeros(8, np.uint32)
    assert lib.nyxhip_assembled_rows(ctx._h, lab.ctypes.data, None, 8) == 0 and lab[:2].tolist() == b2.roi_label.tolist()
    assert lib.nyxhip_assembled_rows(ctx._h, lab.ctypes.data, None, 1) == INVALID_ARG              # too small a max_rows
    ctx.release_volumes()
    assert lib.nyxhip_assembled_rows(ctx._h, lab.ctypes.data, None, 8) == INVALID_ARG              # nothing assembled
    ctx.release_volumes()                                    # releasing twice is fine
    check_assembled(ctx.assemble_volumes_host(I1, L1), b1, vol1, what="after release")
    del a1
    a0 = ctx.assemble_volumes_host(*case("no_label")[:2])
    assert a0.n_roi == 0 and a0.batch.n_roi == 0 and len(a0.labels) == 0 and a0.batch.memory == _abi.MEM_DEVICE


ENTRIES = {
    "volumes": (lambda: (_abi.VFAM_ALL, ()), "volumes", lambda m, s: len(_lib.vol_column_names(m, s))),
    "tex": (lambda: (_abi.VTEX_ALL, (_abi.VolTexSettings(16, 16, 1),)), "volumes_tex", lambda m, s: len(_lib.voltex_column_names(m))),
    "zones": (lambda: (_abi.VZONE_ALL, (_abi.VolZoneSettings(16, 16),)), "volumes_zones", lambda m, s: len(_lib.volzone_column_names(m))),
    "dzones": (lambda: (_abi.VDZ_GLDZM, ()), "volumes_dzones", lambda m, s: len(_lib.voldzone_column_names(m))),
    "shape": (lambda: (_abi.VSHAPE_MORPHOLOGY, ()), "volumes_shape", lambda m, s: len(_lib.volshape_column_names(m))),
}


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("name", list(vc.ENTRY_CASES))
def test_assembled_batch_through_the_entries(ctx, name, entry):
    """The assembled batch, passed unchanged, gives the table of the host batch through the same entry, bit for bit."""
    import torch
    I, L, b, vol = case("entry:" + name)
    make, method, n_cols = ENTRIES[entry]
    (mask, extra), s = make(), _abi.default_settings(64)
    want = getattr(ctx, method + "_host")(b, mask, s, *extra)
    a = ctx.assemble_volumes_host(I, L)
    assert a.n_roi == b.n_roi
    ncol = n_cols(mask, s)
    out = torch.full((a.n_roi, ncol + 1), -1.0, dtype=torch.float64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    getattr(ctx, method + "_device")(a.batch, mask, s, *extra, out.data_ptr(), ncol + 1)
    G = out.cpu().numpy()
    assert (G[:, ncol] == -1.0).all()
    got = np.ascontiguousarray(G[:, :ncol])
    assert got.shape == want.shape and (got.view(np.uint64) == want.view(np.uint64)).all(), (name, entry, np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5])


def test_featurize_routes_agree():
    """Nyxus3DShape(["*3D_ALL*"]): assembly="device" equals assembly="host" as DataFrames, exactly, on a two-volume stack."""
    rng = np.random.default_rng(21)
    I = rng.integers(1, 3000, size=(2, 10, 12, 14), dtype=np.uint32)
    L = np.zeros((2, 10, 12, 14), np.int64)
    L[0, 1:6, 1:7, 1:8] = 5
    L[0, 6:10, 5:12, 6:14] = 2
    L[1, 0:5, 0:6, 0:7] = 5
    L[1, 4:9, 6:11, 7:13] = 70000
    n = Nyxus3DShape(["*3D_ALL*"])
    for k in ("3gldm/greydepth", "3ngtdm/greydepth", "3glrlm/greydepth", "3glszm/greydepth"):
        n.set_metaparam(k + "=16")
    n.set_metaparam("3ngtdm/radius=1")
    host = n.featurize(I, L, assembly="host")
    dev = n.featurize(I, L, assembly="device")
    assert list(host.columns) == list(dev.columns) and len(host) == len(dev) == 4
    for c in host.columns:
        h, d = host[c].to_numpy(), dev[c].to_numpy()
        if h.dtype == np.float64:
            assert (h.view(np.uint64) == d.view(np.uint64)).all(), c
        else:
            assert (h == d).all(), c
    assert n.featurize(I, L).equals(host)                    # the default is the host route
    empty = n.featurize(I, np.zeros_like(L), assembly="device")
    assert len(empty) == 0 and list(empty.columns) == list(host.columns)


def test_unbinned_grey_depth_hint_survives_on_the_device_route():
    rng = np.random.default_rng(22)
    I = rng.integers(1, 60000, size=(1, 6, 6, 6), dtype=np.uint32)
    L = np.ones((1, 6, 6, 6), np.uint32)
    n = Nyxus3DShape(["*3D_GLDM*"])
    for route in ("host", "device"):
        with pytest.raises(_lib.NyxHipError, match=r'set_metaparam\("3gldm/greydepth=<levels>"\)') as ei:
            n.featurize(I, L, assembly=route)
        assert ei.value.code == UNSUPPORTED


def test_refusals(ctx):
    lib = _lib.load()
    buf = np.ones(8, np.uint32)
    out = _abi.Batch3D()

    def rc(shape=(1, 2, 2, 2), di=_abi.U32, dl=_abi.U32, memory=_abi.MEM_HOST, inten=buf.ctypes.data, label=buf.ctypes.data, v=True, o=True):
        vs = _abi.volumes_struct(inten, di, label, dl, shape, memory)
        return lib.nyxhip_assemble_volumes(ctx._h, C.byref(vs) if v else None, C.byref(out) if o else None, None)

    assert rc() == 0 and out.n_roi == 1
    assert rc(v=False) == INVALID_ARG and rc(o=False) == INVALID_ARG
    assert rc(inten=None) == INVALID_ARG and rc(label=None) == INVALID_ARG
    assert rc(di=3) == INVALID_ARG and rc(dl=0) == INVALID_ARG and rc(dl=8) == INVALID_ARG
    assert rc(memory=2) == INVALID_ARG and rc(memory=-1) == INVALID_ARG
    for shape in ((0, 2, 2, 2), (1, 0, 2, 2), (1, 2, 0, 2), (1, 2, 2, 0)):
        assert rc(shape=shape) == INVALID_ARG, shape
    # a side above 65534 (coordinates are 16-bit); 2^32 voxels or more (voxel counts are 32-bit): refused before anything is read
    for shape in ((1, 1, 1, 65535), (1, 1, 65535, 1), (1, 65535, 1, 1)):
        assert rc(shape=shape) == ROI_TOO_LARGE, shape
    assert rc(shape=(1, 65534, 65534, 2)) == UNSUPPORTED and rc(shape=(1, 1, 65536, 65536)) == ROI_TOO_LARGE
    assert b"2^32" in lib.nyxhip_last_error(ctx._h) or b"65534" in lib.nyxhip_last_error(ctx._h)
    # a refused call leaves no batch behind
    assert lib.nyxhip_assembled_rows(ctx._h, None, None, 1 << 20) == INVALID_ARG
    assert rc() == 0 and lib.nyxhip_assembled_rows(ctx._h, None, None, 0) == INVALID_ARG and lib.nyxhip_assembled_rows(ctx._h, None, None, 1) == 0
