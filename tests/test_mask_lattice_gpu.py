"""Every family block keeps its place and its bits under any mask (a row never depends on companions).

One batch (tests/mask_lattice_cases.py: degenerate ROIs, every size class, both table widths, every deferred list) runs through
featurize_device_async with batch AND origins in device memory (nyxhip_featurize_batch_async_at) into a table prefilled with a
sentinel, three columns wider than the mask needs.  After every call: the padding still holds the sentinel, no cell inside does.
  anchor   per setting and family bit alone: the device table equals the host call's bit for bit and holds against the family's
           reference within the bounds that family's own test file uses
  lattice  per setting and group of masks: every family block, selected by name, equals the anchored single-bit table bit for bit
  extrema  stated against derived batch extrema: the same bits
  tiles    the ROIs that fit one 256 x 256 tile through featurize_tiles_host under a 2 MiB device budget: the batch path's rows
The sentinel is told from a value by the anchors: no anchored table holds it."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import caliper_ref, chords_ref, circle_ref, counts, erosion_ref, outline_cases, outline_ref, parity, radial_ref
from tests import mask_lattice_cases as mc
from tests.test_erosion_cpu import mismatches as erosion_mismatches

pytestmark = pytest.mark.gpu

POISON = mc.POISON
DBL_MAX = 1.7976931348623157e308
CORE = [b for b in mc.BITS if b & _abi.FAM_ALL]
CHUNK = 64                                   # masks per parametrised case
GROUPS = mc.masks()
TAIL = mc.FULL & ~(_abi.FAM_ALL & ~(_abi.FAM_SMOMS | _abi.FAM_IMOMS))      # kTailFams: the families without size classes (no large-ROI workspace)


def same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def differing(a, b, names, keys):
    at = np.argwhere(~same(a, b))
    return (len(at), sorted({keys[i] for i, _ in at}), [(names[j], keys[i], a[i, j], b[i, j]) for i, j in at[:10]])


# ---- the device call ------------------------------------------------------------------------------------------------------------------
_DEV = {}


def device_batch(which="lattice"):
    """A batch of the case module and its origins in device memory, built once."""
    if which not in _DEV:
        import torch
        dev = torch.device("cuda", 0)
        b, keys = mc.lattice_batch() if which == "lattice" else mc.late_lane_batch()
        view = {2: np.int16, 4: np.int32, 8: np.int64}
        keep = {k: torch.from_numpy(getattr(b, k).view(view[getattr(b, k).dtype.itemsize])).to(dev)
                for k in ("px_offset", "x", "y", "inten", "bbox_w", "bbox_h", "min_inten", "max_inten", "origin_x", "origin_y")}
        _DEV[which] = dict(b=b, keys=keys, keep=keep, dev=dev)
    return _DEV[which]


def device_call(ctx, mask, s, stated=True, which="lattice"):
    """One featurize_device_async over the batch -> the table without its padding, after the padding and the sentinel were checked."""
    import torch
    d = device_batch(which)
    b, keep = d["b"], d["keep"]
    cb = b.c_struct()
    for k in ("px_offset", "x", "y", "inten", "bbox_w", "bbox_h", "min_inten", "max_inten"):
        setattr(cb, k, keep[k].data_ptr())
    cb.slide_min = None; cb.slide_max = None; cb.memory = _abi.MEM_DEVICE
    if not stated:
        cb.max_px = cb.max_bbox_area = cb.max_inten_range = cb.max_bbox_side = 0
    ncol = ctx.n_columns(mask, s)
    ld = ncol + 3
    out = torch.full((b.n_roi, ld), POISON, dtype=torch.float64, device=d["dev"])
    ctx.featurize_device_async(cb, mask, s, out.data_ptr(), ld, keep["origin_x"].data_ptr(), keep["origin_y"].data_ptr())
    ctx.sync()
    T = out.cpu().numpy()
    assert (T[:, ncol:] == POISON).all(), (hex(mask), "the padding was written")
    unwritten = np.argwhere(T[:, :ncol] == POISON)
    if len(unwritten):
        names = _lib.column_names(mask, s)
        raise AssertionError((hex(mask), "never written", [(names[j], d["keys"][i]) for i, j in unwritten[:10]]))
    return np.ascontiguousarray(T[:, :ncol])


_ANCHOR = {}


def anchor(ctx, skey, bit):
    """The single-bit table of the device call, computed once per setting."""
    if (skey, bit) not in _ANCHOR:
        _ANCHOR[skey, bit] = device_call(ctx, bit, mc.SETTINGS[skey]())
    return _ANCHOR[skey, bit]


# ---- the references -------------------------------------------------------------------------------------------------------------------
_REF = {}


def contours():
    if "K" not in _REF:
        _REF["K"] = radial_ref.contours_of(mc.lattice_batch()[0])
    return _REF["K"]


def ref_table(what):
    """The CPU restatements of the families without an oracle entry, computed once (none of them reads the settings but soft_nan)."""
    if what not in _REF:
        b = mc.lattice_batch()[0]
        if what == "caliper":
            _REF[what] = caliper_ref.table(b, soft_nan=mc.SOFT_NAN)
        elif what == "chords":
            _REF[what] = chords_ref.table(b)
        elif what == "erosion":
            _REF[what] = erosion_ref.table(b)
        elif what == "outline":
            _REF[what] = outline_ref.outline_table(b, contours())
        elif what == "circle":
            _REF[what] = circle_ref.table(b, contours())[:, :5]
        elif what == "radial":
            _REF[what] = radial_ref.radial_table(b, contours(), with_dst2=True)
    return _REF[what]


def sub_batch(b, rows):
    off = b.px_offset.astype(np.int64)
    px = np.concatenate([np.arange(off[r], off[r + 1]) for r in rows])
    n = np.array([off[r + 1] - off[r] for r in rows])
    return _abi.HostBatch(b.roi_label[rows], np.concatenate([[0], np.cumsum(n)]), b.x[px], b.y[px], b.inten[px], b.bbox_w[rows], b.bbox_h[rows],
                          b.min_inten[rows], b.max_inten[rows], origin_x=b.origin_x[rows], origin_y=b.origin_y[rows])


def check_core(G, bit, s, b, keys):
    """oracle.pyoracle under the bounds of tests/test_soft_nan_gpu.py; Gabor on the rows whose boxes stay within 64 pixels (the CPU oracle
    is slow beyond: tests/test_large_rois_gpu.py pins those)."""
    rows = np.arange(b.n_roi)
    if bit == _abi.FAM_GABOR:
        rows = np.flatnonzero(np.maximum(b.bbox_w, b.bbox_h) <= 64)
        assert len(rows) >= 8
        b = sub_batch(b, rows)
    names = _lib.column_names(bit, s)
    O = po.oracle_featurize(b, bit, s)
    bad = parity.compare_tables(G[rows], O, names, batch=b) + counts.compare_counts(G[rows], O, names) + counts.compare_tight(G[rows], O, names)
    assert not bad, "\n".join(bad[:20])
    if bit == _abi.FAM_GABOR:
        assert same(G[rows], O).all()                                          # counts: bit for bit (tests/test_soft_nan_gpu.py)
    return O


def check_tail(G, bit, b, keys):
    """The restatements, each as the family's own GPU test compares with it."""
    F = _abi
    if bit & F.FAM_CALIPER:                                                    # tests/test_caliper_gpu.py: the same bits as the restatement
        sl = {F.FAM_FERET: slice(0, 8), F.FAM_MARTIN: slice(8, 14), F.FAM_NASSENSTEIN: slice(14, 20)}[bit]
        W = ref_table("caliper")[:, sl]
        assert same(G, W).all(), differing(G, W, caliper_ref.NAMES[sl], keys)
    elif bit == F.FAM_CHORDS:                                                  # tests/test_chords_gpu.py: the same bits
        W = ref_table("chords")
        assert same(G, W).all(), differing(G, W, chords_ref.NAMES, keys)
    elif bit in (F.FAM_ELLIPSE, F.FAM_EROSION):
        # tests/test_erosion_gpu.py: every column but ORIENTATION (atan) bit for bit; ORIENTATION at parity.REL_TOL where the
        # restatement's exact sums say it is no rounding noise (erosion_ref.compared)
        W = ref_table("erosion")
        if bit == F.FAM_EROSION:
            assert same(G, W[:, 6:]).all(), differing(G, W[:, 6:], erosion_ref.EROSION, keys)
        else:
            ex = [0, 1, 2, 3, 5]
            assert same(G[:, ex], W[:, ex]).all(), differing(G[:, ex], W[:, ex], [erosion_ref.ELLIPSE[c] for c in ex], keys)
            cmp_ = np.array([erosion_ref.compared(x, y, W[r, 4]) for r, x, y in erosion_ref.rois_of(b)])
            bad = erosion_mismatches(np.hstack([G, W[:, 6:]]), W, cmp_)
            assert not bad, "\n".join(bad[:10])
    elif bit in (F.FAM_FRACTAL, F.FAM_EULER, F.FAM_ROI_RADIUS):
        # tests/test_outline_gpu.py: outline_cases.mismatches at parity.REL_TOL (NaN in the restatement: undefined in the reference);
        # Euler number, radius max and median: the same bits
        W = ref_table("outline")
        cols = [j for j, n in enumerate(outline_cases.NAMES) if n in _lib.column_names(bit, mc.settings_a())]
        full = W.copy()
        full[:, cols] = G
        bad = outline_cases.mismatches(full, W, parity.REL_TOL)
        assert not bad, "\n".join(bad[:10])
        for k, j in enumerate(cols):
            if outline_cases.NAMES[j] in outline_cases.EXACT:
                use = ~np.isnan(W[:, j])
                assert (G[use, k] == W[use, j]).all()
    elif bit in (F.FAM_CIRCLES, F.FAM_GEODETIC):                               # tests/test_circle_gpu.py: the same bits
        W = ref_table("circle")[:, :3] if bit == F.FAM_CIRCLES else ref_table("circle")[:, 3:]
        assert same(G, W).all(), differing(G, W, circle_ref.NAMES[:3] if bit == F.FAM_CIRCLES else circle_ref.NAMES[3:], keys)
    elif bit == F.FAM_RADIAL:
        # tests/test_radial_gpu.py: FRAC_AT_D and MEAN_FRAC exactly, RADIAL_CV at parity.REL_TOL, on the rows the reference defines
        # (a centre at distance 0 from the contour is undefined there)
        W, D = ref_table("radial")
        use = np.array([d is None or d != 0 for d in D])
        assert use.sum() >= b.n_roi - 6, D
        bad = parity.compare_tables(G[use], W[use], radial_ref.NAMES, exact=radial_ref.EXACT)
        assert not bad, bad[:10]
        ex = [i for i, n in enumerate(radial_ref.NAMES) if n in radial_ref.EXACT]
        assert same(G[use][:, ex], W[use][:, ex]).all()
    else:
        raise AssertionError(hex(bit))


# ---- anchor ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit", [pytest.param(b, id=mc.NAME_OF[b]) for b in mc.BITS])
@pytest.mark.parametrize("skey", list(mc.SETTINGS))
def test_anchor(hip_ctx, skey, bit):
    s = mc.SETTINGS[skey]()
    b, keys = mc.lattice_batch()
    names = _lib.column_names(bit, s)
    G = anchor(hip_ctx, skey, bit)
    assert not (G == POISON).any()                                             # (device_call has checked it: no legitimate value is the sentinel)
    host = hip_ctx.featurize_host(b, bit, s)
    assert same(G, host).all(), differing(G, host, names, keys)
    if bit & _abi.FAM_ALL:
        O = check_core(G, bit, s, b, keys)
        assert not (O == POISON).any()
        if bit not in (_abi.FAM_INTENSITY, _abi.FAM_SMOMS, _abi.FAM_IMOMS, _abi.FAM_GABOR):
            assert (O == mc.SOFT_NAN).any()                                    # the degenerate rows say something at this soft_nan
    else:
        check_tail(G, bit, b, keys)


def test_the_batch_reaches_every_launch_path(hip_ctx):
    """The classes as launched (nyxhip_launch_report) against the restated class rule; the five deferred lists and the degenerate rows
    are asserted by mc.lattice_batch() itself."""
    b, keys = mc.lattice_batch()
    s = mc.settings_a()
    for mask in (_abi.FAM_INTENSITY | _abi.FAM_GLCM, mc.FULL):
        hip_ctx.featurize_host(b, mask, s)
        rep = hip_ctx.launch_report()
        print(hex(mask), "launch groups:", mc.check_launch_report(rep, b))
    L = mc.listed(b)
    print({k: [keys[r] for r in v] for k, v in L.items()})
    assert sorted({c // 2 for c in mc.classes(b)}) == [0, 1, 2, 3, 4]


def test_unassigned_bits_are_bad_masks(hip_ctx):
    b = sub_batch(mc.lattice_batch()[0], np.arange(5))
    s = mc.settings_a()
    for k in mc.UNASSIGNED:
        for good in (0, _abi.FAM_EULER, mc.FULL):
            with pytest.raises(_lib.NyxHipError) as ei:
                hip_ctx.featurize_host(b, good | (1 << k), s)
            assert ei.value.code == 1, (k, hex(good))                          # NYXHIP_ERR_INVALID_ARG


# ---- lattice --------------------------------------------------------------------------------------------------------------------------
def check_blocks(ctx, skey, s, mask, T, keys, what=""):
    names = _lib.column_names(mask, s)
    col = {n: j for j, n in enumerate(names)}
    assert len(col) == len(names) == T.shape[1]
    seen = 0
    for bit in mc.bits_of(mask):
        sub = _lib.column_names(bit, s)
        A = anchor(ctx, skey, bit)
        block = T[:, [col[n] for n in sub]]
        keep = [j for j, n in enumerate(sub) if n not in mc.MASK_DEPENDENT]
        assert same(block[:, keep], A[:, keep]).all(), (what, hex(mask), mc.NAME_OF[bit], differing(block, A, sub, keys))
        seen += len(sub)
    assert seen == len(names)


def _cases():
    out = []
    for g, ms in GROUPS.items():
        if g == "singles":
            continue                                                           # (the anchors themselves)
        for k in range(0, len(ms), CHUNK):
            out.append(pytest.param(g, k, id=f"{g}-{k // CHUNK}"))
    return out


@pytest.mark.parametrize("group,start", _cases())
@pytest.mark.parametrize("skey", list(mc.SETTINGS))
def test_lattice(hip_ctx, skey, group, start):
    s = mc.SETTINGS[skey]()
    keys = mc.lattice_batch()[1]
    for mask in GROUPS[group][start:start + CHUNK]:
        check_blocks(hip_ctx, skey, s, mask, device_call(hip_ctx, mask, s), keys)


@pytest.mark.parametrize("skey", list(mc.SETTINGS))
def test_lattice_with_the_deferred_lists_in_chunks(hip_ctx, skey, monkeypatch):
    """The masks of the interleave group that hold no size-class family (a 1 MiB budget is for the deferred lists here, not for the
    large-ROI workspaces) under NYXHIP_LARGE_BUDGET_MB=1: the contour list of this batch takes more than one chunk (asserted from the
    stride the launcher computes), with column bases that are not those of the family alone.  Many chunks per owner:
    tests/test_deferred_lists_gpu.py."""
    s = mc.SETTINGS[skey]()
    b, keys = mc.lattice_batch()
    w, h = b.bbox_w.astype(np.int64), b.bbox_h.astype(np.int64)
    stride = (int((w * h).max()) + 4 * int(max(w.max(), h.max())) + 4 + 255) & ~255
    n_listed = len(mc.listed(b)["ContourPlaneBig"])
    assert 1 <= (1 << 20) // stride < n_listed, (stride, n_listed)
    todo = [m for m in GROUPS["interleave"] if not (m & ~TAIL)]
    assert len(todo) >= 3 * 128
    monkeypatch.setenv("NYXHIP_LARGE_BUDGET_MB", "1")
    for mask in todo[list(mc.SETTINGS).index(skey)::2]:                                          # every other mask per setting: both settings cover the group
        check_blocks(hip_ctx, skey, s, mask, device_call(hip_ctx, mask, s), keys, "1 MiB budget")


def test_contour_families_wait_for_every_glcm_launch(hip_ctx):
    """The `after_all` join of launch_device_all: the finishing kernel of the large classes (roi_large.hip) zeroes its rows from column 0
    across the columns between the intensity block and GLCM, at the end of a chain on a lane.  Here that chain is long (frames with
    planes of millions of cells) and the kernels of the families behind the intensity block are quick (a few thousand pixels), so a
    launch order that lets them run beside the chain loses their values to the zeroing."""
    s = mc.settings_b()
    b, keys = mc.late_lane_batch()
    GLCM = _abi.FAM_GLCM
    for bit in mc.BEHIND_INTENSITY:
        alone = device_call(hip_ctx, bit, s, which="late")
        for mask in (bit | GLCM, bit | GLCM | _abi.FAM_INTENSITY):
            T = device_call(hip_ctx, mask, s, which="late")
            names = _lib.column_names(mask, s)
            block = T[:, [names.index(n) for n in _lib.column_names(bit, s)]]
            assert same(block, alone).all(), (hex(mask), mc.NAME_OF[bit], differing(block, alone, _lib.column_names(bit, s), keys))


# ---- stated against derived extrema ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skey", list(mc.SETTINGS))
def test_derived_extrema_give_the_same_bits(hip_ctx, skey):
    s = mc.SETTINGS[skey]()
    keys = mc.lattice_batch()[1]
    for mask in [mc.FULL] + GROUPS["random"][:6]:
        stated = device_call(hip_ctx, mask, s)
        derived = device_call(hip_ctx, mask, s, stated=False)
        assert same(stated, derived).all(), (hex(mask), differing(derived, stated, _lib.column_names(mask, s), keys))
        check_blocks(hip_ctx, skey, s, mask, derived, keys, "derived extrema")


# ---- the tile path --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skey", list(mc.SETTINGS))
def test_tile_path(hip_ctx, skey):
    """featurize_tiles_host over a stack of three under a 2 MiB device budget against the batch path's rows of the same ROIs at their
    in-tile origins; the masks walk the window decision of nyxhip_tiles.hip (INTENSITY / GLCM alone against anything else)."""
    s = mc.SETTINGS[skey]()
    b, keys = mc.lattice_batch()
    it, lab, rows = mc.tile_subset(b, keys)
    # roi_cloud_kernel (tile_assembly.hip) writes an ROI's cloud in row-major order of its window; sums close in the order of the cloud
    # and the radial centre's tie-break follows it, so the batch holds the same order
    rois = []
    for r in rows:
        ys, xs = np.nonzero(lab == r + 1)
        rois.append(dict(label=r + 1, x=xs, y=ys, inten=it[ys, xs], slide_min=DBL_MAX, slide_max=-DBL_MAX))
    tb = _abi.batch_from_rois(rois)
    assert np.array_equal(tb.bbox_w, b.bbox_w[rows]) and np.array_equal(tb.bbox_h, b.bbox_h[rows]) and (tb.origin_x < 256).all()
    tkeys = [keys[r] for r in rows]
    I, M = np.stack([it] * 3), np.stack([lab] * 3)
    todo = [mc.FULL, _abi.FAM_INTENSITY, _abi.FAM_GLCM, _abi.FAM_INTENSITY | _abi.FAM_GLCM] + GROUPS["glcm_span"] + GROUPS["random"][6:18]
    for mask in todo:
        want = hip_ctx.featurize_host(tb, mask, s)
        ti, labels, T = hip_ctx.featurize_tiles_host(I, M, mask, s, max_device_bytes=2 << 20)
        assert list(labels) == list(tb.roi_label) * 3 and list(ti) == [k for k in range(3) for _ in rows]
        W = np.tile(want, (3, 1))
        assert same(T, W).all(), (hex(mask), differing(T, W, _lib.column_names(mask, s), tkeys * 3))
