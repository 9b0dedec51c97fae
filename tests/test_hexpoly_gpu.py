"""POLYGONALITY_AVE, HEXAGONALITY_AVE, HEXAGONALITY_STDDEV on the GPU (nyxhip_hexpoly_batch / nyxhip_hexpoly_tiles), class
NyxusAllMorphology and the group *ALL_MORPHOLOGY*.

What a row is held to (tests/hexpoly_ref.py is pinned to the reference's class bit for bit by tests/test_hexpoly_cpu.py):
  equal bits        every row whose NUM_NEIGHBORS is at most 128: the six inputs have the reference's bits (their own tests), and the
                    closing is IEEE +, -, *, / and square roots, unfused, with tan(M_PI / k) from the host's libm
  parity.REL_TOL    rows beyond the tangent table (the device's tan): |got - want| <= REL_TOL * max(|want|, 1).  The floor of 1 is
                    there because a score is 10 x a mean of terms whose rounding error is absolute at scale >= 1; a score near 0 has no
                    relative accuracy in the reference either.  NaN and infinities stand in the same places; -1 rows are exactly -1."""
import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import hexpoly_cases as hc, hexpoly_ref as hr, morph_cases, morph_ref, neighbors_cases as nc, neighbors_ref as nr, parity

pytestmark = pytest.mark.gpu

GOLD = hc.golden()
_ROWS = {}


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def settings():
    return _abi.default_settings(64)


def rows(ctx, name):
    """The three columns of a case through the batch entry on a host batch, computed once and shared."""
    if name not in _ROWS:
        _ROWS[name] = ctx.hexpoly_host(hc.batch(name), hc.radius(name), settings())
    return _ROWS[name]


def check_against(got, want, neighbors, tag):
    """Rows within the tangent table: the bits of `want`.  Rows beyond it: the stated bound, non-finite values in the same places."""
    assert got.shape == want.shape, tag
    inside = np.asarray(neighbors) <= hr.TAN_TABLE_CAP
    diff = np.abs(got - want)
    print(f"{tag}: {len(got)} rows ({int((~inside).sum())} beyond the tangent table); largest difference per column "
          f"{dict(zip(hr.NAMES, np.nan_to_num(np.where(np.isfinite(diff), diff, 0.0)).max(0).tolist()))}")
    bad = [r for r in np.nonzero(inside)[0] if not hr.same_bits(got[r], want[r])]
    assert not bad, (tag, [(int(r), got[r].tolist(), want[r].tolist()) for r in bad[:6]])
    g, w = got[~inside], want[~inside]
    fin = np.isfinite(w)
    assert (np.isnan(g) == np.isnan(w)).all() and (g[~fin & ~np.isnan(w)] == w[~fin & ~np.isnan(w)]).all(), tag
    assert ((g == -1) == (w == -1)).all(), tag
    assert (np.abs(g[fin] - w[fin]) <= parity.REL_TOL * np.maximum(np.abs(w[fin]), 1.0)).all(), (tag, g[fin], w[fin])
    assert hr.same_bits(g[:, 1:], w[:, 1:]), tag                             # the tangent serves POLYGONALITY_AVE alone


def device_rows(ctx, b, distance, stated, ld_extra=2):
    """The batch entry on a batch in device memory (extrema stated or derived) with a table wider than three columns."""
    import torch
    dev = torch.device("cuda", 0)
    view = {2: np.int16, 4: np.int32, 8: np.int64}
    keys = ("roi_label", "px_offset", "x", "y", "inten", "bbox_w", "bbox_h")
    keep = {k: torch.from_numpy(np.ascontiguousarray(getattr(b, k)).view(view[np.asarray(getattr(b, k)).dtype.itemsize])).to(dev) for k in keys}
    ox = oy = io = None
    if b.origin_x is not None:
        ox, oy = (torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev) for a in (b.origin_x, b.origin_y))
    if b.image_offset is not None:
        io = torch.from_numpy(np.ascontiguousarray(b.image_offset, np.uint64).view(np.int64)).to(dev)
    cb = _abi.Batch()
    cb.n_roi = b.n_roi
    for k, t in keep.items():
        setattr(cb, k, t.data_ptr())
    cb.memory = _abi.MEM_DEVICE
    if stated:
        h = b.c_struct()
        cb.max_px, cb.max_bbox_area, cb.max_bbox_side = h.max_px, h.max_bbox_area, h.max_bbox_side
    ld = _abi.HEXPOLY_COLS + ld_extra
    out = torch.full((b.n_roi, ld), -7.0, dtype=torch.float64, device=dev)
    ctx.hexpoly_device(cb, ox.data_ptr() if ox is not None else None, oy.data_ptr() if oy is not None else None,
                       io.data_ptr() if io is not None else None, len(b.image_offset) - 1 if io is not None else 0, distance, settings(),
                       out.data_ptr(), ld)
    G = out.cpu().numpy()
    assert (G[:, _abi.HEXPOLY_COLS:] == -7.0).all()                          # nothing is written beyond the three columns
    return np.ascontiguousarray(G[:, :_abi.HEXPOLY_COLS])


@pytest.mark.parametrize("name", list(hc.CASES))
def test_host_batch_rows_have_the_bits_of_the_reference(hip_ctx, name):
    X, want = GOLD[name]
    check_against(rows(hip_ctx, name), want, X[:, 2], name)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_device_batches_give_the_rows_of_host_batches(hip_ctx, name):
    b = hc.batch(name)
    for stated in (True, False):
        assert same(device_rows(hip_ctx, b, hc.radius(name), stated), rows(hip_ctx, name)), (name, stated)


def test_rows_beyond_the_tangent_table_are_met_and_the_gates_are_exact(hip_ctx):
    X, want = GOLD["beyond_table"]
    got = rows(hip_ctx, "beyond_table")
    assert X[0, 2] == 400 and np.isfinite(got[0]).all() and got[0, 0] != -1
    for name in ("low_counts", "no_contour", "deferred", "three_images"):
        T, W = rows(hip_ctx, name), GOLD[name][1]
        gated = (W == -1).all(axis=1)
        assert gated.any() and (T[gated] == -1.0).all() and (T[~gated] != -1.0).all(), name
    b = hc.batch("hex_discs")
    mid = [int(np.nonzero(np.asarray(b.roi_label) == lab)[0][0]) for lab in hc.HEX_MIDDLE]
    assert rows(hip_ctx, "hex_discs")[mid, 1].min() > rows(hip_ctx, "lattice")[:, 1].max()    # packed discs are more hexagonal than boxes


@pytest.mark.parametrize("name", ["lattice", "needle", "beyond_table", "deferred", "three_images", "far"])
def test_closing_kernel_alone_over_the_devices_own_inputs(hip_ctx, name):
    """The six columns as the three older entries give them on the same batch, through hexpoly_ref.closing: the bits of the entry's rows.
    With the first test this separates "the inputs moved" from "the formula moved"."""
    s = settings()
    b = hc.batch(name)
    nb = hip_ctx.neighbors_host(b, hc.radius(name), s)[:, 0]
    mo = hip_ctx.morph_host(b, _abi.MORPH_CONTOUR | _abi.MORPH_HULL, s)
    fe = hip_ctx.featurize_host(b, _abi.FAM_FERET, s)
    X = GOLD[name][0]
    own = np.column_stack([X[:, 0], X[:, 1], nb, mo[:, 0], mo[:, 8], fe[:, 2], fe[:, 3]])
    assert _lib.morph_column_names(6)[0] == "PERIMETER" and _lib.morph_column_names(6)[8] == "CONVEX_HULL_AREA"
    assert _lib.column_names(_abi.FAM_FERET, s)[2:4] == ["STAT_FERET_DIAM_MIN", "STAT_FERET_DIAM_MAX"]
    live = X[:, 1] > 0                                                       # (a ROI without a contour: its Feret columns hold the soft NaN)
    assert hr.same_bits(own[live], X[live]), np.argwhere(own != X)[:6]       # the inputs have the reference's bits
    check_against(rows(hip_ctx, name), hr.closing_rows(own), nb, name + " (device inputs)")


@pytest.mark.parametrize("name", [n for n, c in hc.CASES.items() if c[2] is None])
def test_tile_entry_gives_the_bits_of_the_batch_entry(hip_ctx, name):
    s = settings()
    I, M = hc.stack(name)
    b = hc.batch(name)
    tiles, labels, table = hip_ctx.hexpoly_tiles_host(I, M, hc.radius(name), s)
    assert labels.tolist() == np.asarray(b.roi_label).tolist()
    assert tiles.tolist() == np.repeat(np.arange(len(M)), np.diff(b.image_offset.astype(np.int64))).tolist()
    assert same(table, rows(hip_ctx, name)), name
    if len(M) > 1:                                                           # a budget of a tile or so: the stack in several chunks
        _, _, chunked = hip_ctx.hexpoly_tiles_host(I, M, hc.radius(name), s, max_device_bytes=200_000)
        assert same(chunked, rows(hip_ctx, name))


def test_a_row_has_the_same_bits_whatever_shares_its_call(hip_ctx):
    s = settings()
    labs = hc.images("three_images")
    full = rows(hip_ctx, "three_images")
    for k, (lo, hi) in enumerate(nr.image_ranges(hc.batch("three_images"))):
        alone = hip_ctx.hexpoly_host(nc.batch_of_images(labs[k:k + 1], seed0=500 + k), 5, s)
        assert same(alone, full[lo:hi]), k
    one = hc.batch("lattice")
    one.image_offset = None                                                  # image_offset None: one image
    assert same(hip_ctx.hexpoly_host(one, 5, s), rows(hip_ctx, "lattice"))
    assert same(hip_ctx.hexpoly_host(hc.batch("hex_discs"), 5, s), rows(hip_ctx, "hex_discs"))         # repeatable, other calls in between
    wider = hip_ctx.hexpoly_host(hc.batch("low_counts"), 20, s)              # the distance takes effect: the row of four sees each other
    assert (wider[:4] != -1).all() and (wider[4] == -1).all() and (rows(hip_ctx, "low_counts") == -1).all()
    assert hr.same_bits(wider, hr.table(hc.batch("low_counts"), 20))


def test_older_entries_keep_their_bits_around_a_hexpoly_call(hip_ctx):
    """nyxhip_neighbors_batch and nyxhip_morph_batch after the split of their device functions: the recorded values of their own fixtures,
    and the same bits before and after a hexpoly call on the same context (the contour workspace and the neighbor tables are shared)."""
    s = settings()
    nb_gold, mo_gold = nc.golden(), morph_cases.golden()
    exact_nb = [i for i, n in enumerate(nr.NAMES) if n in nr.EXACT]
    exact_mo = [i for i, n in enumerate(morph_ref.NAMES) if n not in morph_ref.ROUNDED]
    for name, radius in (("contacts", 5), ("ring", 12), ("three_images", 5)):
        before = hip_ctx.neighbors_host(nc.batch(name), radius, s)
        hip_ctx.hexpoly_host(hc.batch("deferred"), 5, s)
        after = hip_ctx.neighbors_host(nc.batch(name), radius, s)
        want = nb_gold[(name, radius)][:, :9]
        assert same(before, after) and (before[:, exact_nb] == want[:, exact_nb]).all(), name
        assert (np.abs(before - want) <= parity.REL_TOL * np.abs(want)).all(), name
    for name in ("mixed", "small", "placed"):
        before = hip_ctx.morph_host(morph_cases.batch(name), _abi.MORPH_ALL, s)
        hip_ctx.hexpoly_host(hc.batch("lattice"), 5, s)
        after = hip_ctx.morph_host(morph_cases.batch(name), _abi.MORPH_ALL, s)
        want = mo_gold[name]["table"]
        assert same(before, after) and hr.same_bits(before[:, exact_mo], want[:, exact_mo]), name


def test_errors(hip_ctx):
    s = settings()
    b = hc.batch("lattice")
    good = rows(hip_ctx, "lattice")
    for bad_distance in (0, -3):
        with pytest.raises(_lib.NyxHipError) as ei:
            hip_ctx.hexpoly_host(b, bad_distance, s)
        assert ei.value.code == 1
        with pytest.raises(_lib.NyxHipError) as ei:
            hip_ctx.hexpoly_tiles_host(*hc.stack("lattice"), bad_distance, s)
        assert ei.value.code == 1
    with pytest.raises(_lib.NyxHipError) as ei:
        hip_ctx.hexpoly_host(b, 46341, s)
    assert ei.value.code == 4                                                # NYXHIP_ERR_UNSUPPORTED
    with pytest.raises(_lib.NyxHipError) as ei:
        hip_ctx.hexpoly_tiles_host(*hc.stack("lattice"), 46341, s)
    assert ei.value.code == 4
    d = hc.batch("lattice")
    lab = np.asarray(d.roi_label).copy()
    lab[[3, 4]] = lab[[4, 3]]                                                # descending labels inside an image
    d.roi_label = lab
    with pytest.raises(_lib.NyxHipError) as ei:
        hip_ctx.hexpoly_host(d, 5, s)
    assert ei.value.code == 1
    import ctypes as C
    empty = _abi.Batch()                                                     # an empty batch is OK
    empty.n_roi = 0; empty.memory = _abi.MEM_HOST
    out = np.full(3, -7.0)
    assert _lib.load().nyxhip_hexpoly_batch(hip_ctx._h, C.byref(empty), None, None, None, 0, 5, C.byref(s), out.ctypes.data, 3) == 0
    assert (out == -7.0).all()
    assert same(hip_ctx.hexpoly_host(b, 5, s), good)                         # the context serves the next call


def test_through_nyxus_all_morphology(hip_ctx):
    api = hc.api_expected()
    I, M = hc.stack(api["case"])
    want = np.asarray(api["numeric"])
    nyx = nyxus_amd.NyxusAllMorphology(["*ALL_MORPHOLOGY*"], neighbor_distance=api["neighbor_distance"])
    df = nyx.featurize(I, M)
    assert list(df.columns[4:]) == api["all_morphology"] and len(df.columns) == 4 + 108 and df["ROI_label"].tolist() == api["labels"]
    got = df[api["columns"]].to_numpy()
    assert (np.abs(got - want) <= parity.REL_TOL * np.maximum(np.abs(want), 1.0)).all() and ((got == -1) == (want == -1)).all()
    assert same(np.ascontiguousarray(got), np.where(np.isfinite(rows(hip_ctx, api["case"])), rows(hip_ctx, api["case"]), 0.0))
    # the other 105 columns are those of the parent class
    rest = [c for c in api["all_morphology"] if c not in api["columns"]]
    parent = nyxus_amd.NyxusMorphology(rest, neighbor_distance=api["neighbor_distance"]).featurize(I, M)
    assert same(df[rest].to_numpy(), parent[rest].to_numpy())
    # a mixed request comes back in enum order, each column that of the call that owns it
    mixed = nyxus_amd.NyxusAllMorphology(["MEAN", "HEXAGONALITY_AVE", "PERIMETER", "GLCM_ASM"], neighbor_distance=api["neighbor_distance"]).featurize(I, M)
    assert [c.rsplit("_", 1)[0] if c.startswith("GLCM_ASM_") else c for c in mixed.columns[4:]][:4] == ["MEAN", "PERIMETER", "HEXAGONALITY_AVE", "GLCM_ASM"]
    assert all(c.startswith("GLCM_ASM_") for c in mixed.columns[7:])
    assert same(mixed["HEXAGONALITY_AVE"].to_numpy(), df["HEXAGONALITY_AVE"].to_numpy()) and same(mixed["PERIMETER"].to_numpy(), df["PERIMETER"].to_numpy())
    only = nyxus_amd.NyxusAllMorphology(["HEXAGONALITY_STDDEV"], neighbor_distance=2).featurize(I, M)
    assert list(only.columns[4:]) == ["HEXAGONALITY_STDDEV"] and (only["HEXAGONALITY_STDDEV"].to_numpy() != df["HEXAGONALITY_STDDEV"].to_numpy()).any()
