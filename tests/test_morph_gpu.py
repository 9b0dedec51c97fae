"""The 2-D morphology entries on the GPU: the HIP rows against values recorded from the reference's own classes (tests/golden/morph)
-- equal bits for 38 columns, parity.REL_TOL for COMPACTNESS, EDGE_MEAN_INTENSITY and EDGE_STDDEV_INTENSITY, which the reference forms
with an on-line update --, and against themselves across every way a row can be requested: a row has the same bits whichever mask,
launch, call, entry or batch served it."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import morph_cases, morph_ref, parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = _abi.MORPH_ALL
N = morph_ref.NAMES
ROUNDED = [N.index(c) for c in morph_ref.ROUNDED]
EXACT = [i for i in range(41) if i not in ROUNDED]
GOLD = morph_cases.golden()
_ROWS = {}


def same(a, b):
    """Equal bits (the tables hold no NaN; +inf equals +inf)."""
    return a.shape == b.shape and bool((np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)).all())


def rows(ctx, name):
    """The 41 columns of a case, computed once and shared."""
    if name not in _ROWS:
        _ROWS[name] = ctx.morph_host(morph_cases.batch(name), ALL, _abi.default_settings(64))
    return _ROWS[name]


@pytest.mark.parametrize("name", list(morph_cases.CASES))
def test_hip_rows_match_the_reference_classes(hip_ctx, name):
    want = GOLD[name]["table"]
    got = rows(hip_ctx, name)
    assert got.shape == want.shape and not np.isnan(got).any()
    with np.errstate(invalid="ignore"):
        rel = np.where(got == want, 0.0, np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
    print(f"{name}: {len(got)} ROIs; largest relative difference per column: " + ", ".join(f"{N[c]} {rel[:, c].max():.3g}" for c in range(41) if rel[:, c].max() > 0))
    bad = got[:, EXACT].view(np.uint64) != want[:, EXACT].view(np.uint64)        # +inf in the same places included
    assert not bad.any(), [(int(r), N[EXACT[c]], got[r, EXACT[c]], want[r, EXACT[c]]) for r, c in np.argwhere(bad)[:8]]
    for c in ROUNDED:
        assert (np.abs(got[:, c] - want[:, c]) <= parity.REL_TOL * np.abs(want[:, c])).all(), (N[c], got[:, c], want[:, c])


def test_every_subset_of_the_four_bits(hip_ctx):
    s = _abi.default_settings(64)
    for name in ("small", "shapes", "words", "mixed"):
        b, full = morph_cases.batch(name), rows(hip_ctx, name)
        for m in range(1, 16):
            got = hip_ctx.morph_host(b, m, s)
            assert same(got, full[:, morph_ref.columns_of(m)]), (name, m)


def _device_rows(ctx, b, mask, stated, origins=True, ld_extra=3):
    import torch
    dev = torch.device("cuda", 0)
    view = {2: np.int16, 4: np.int32, 8: np.int64}
    keep = {k: torch.from_numpy(getattr(b, k).view(view[getattr(b, k).dtype.itemsize])).to(dev) for k in ("px_offset", "x", "y", "inten", "bbox_w", "bbox_h")}
    ox = oy = None
    if origins and b.origin_x is not None:
        ox, oy = (torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev) for a in (b.origin_x, b.origin_y))
    cb = _abi.Batch()
    cb.n_roi = b.n_roi
    for k, t in keep.items():
        setattr(cb, k, t.data_ptr())
    cb.memory = _abi.MEM_DEVICE
    if stated:
        h = b.c_struct()
        cb.max_px, cb.max_bbox_area, cb.max_bbox_side = h.max_px, h.max_bbox_area, h.max_bbox_side
    ncol = len(morph_ref.columns_of(mask))
    out = torch.full((b.n_roi, ncol + ld_extra), -1.0, dtype=torch.float64, device=dev)
    ctx.morph_device(cb, ox.data_ptr() if ox is not None else None, oy.data_ptr() if oy is not None else None, mask, _abi.default_settings(64),
                     out.data_ptr(), ncol + ld_extra)
    G = out.cpu().numpy()
    assert (G[:, ncol:] == -1.0).all()                                       # nothing is written beyond the mask's columns
    return G[:, :ncol]


def test_host_and_device_batches_agree(hip_ctx):
    for name in ("mixed", "placed", "words"):
        b = morph_cases.batch(name)
        for stated in (True, False):
            assert same(_device_rows(hip_ctx, b, ALL, stated), rows(hip_ctx, name)), (name, stated)
    b = morph_cases.batch("mixed")
    assert same(_device_rows(hip_ctx, b, _abi.MORPH_HULL | _abi.MORPH_EXTREMA, False), rows(hip_ctx, "mixed")[:, morph_ref.columns_of(12)])


def test_rows_are_repeatable_and_independent_of_the_batch(hip_ctx):
    s = _abi.default_settings(64)
    for name in ("small", "collinear", "ties", "mixed"):
        assert same(hip_ctx.morph_host(morph_cases.batch(name), ALL, s), rows(hip_ctx, name)), name
    rois, mixed = morph_cases.mixed(), rows(hip_ctx, "mixed")
    for r in range(len(rois)):                                               # each ROI alone: other LDS carve-outs, the ring and the comb without the bulk
        assert same(hip_ctx.morph_host(_abi.batch_from_rois(rois[r:r + 1]), ALL, s), mixed[r:r + 1]), r
    assert same(rows(hip_ctx, "long_comb"), mixed[morph_cases.MIXED_COMB:morph_cases.MIXED_COMB + 1])
    assert same(rows(hip_ctx, "ring"), mixed[morph_cases.MIXED_RING:morph_cases.MIXED_RING + 1])
    wide = morph_cases.words()                                               # 1025 columns: the list launch over global tables, alone and in the batch
    assert same(hip_ctx.morph_host(_abi.batch_from_rois(wide[-1:]), ALL, s), rows(hip_ctx, "words")[-1:])


def test_rows_do_not_depend_on_the_pixel_order(hip_ctx):
    s = _abi.default_settings(64)
    rng = np.random.default_rng(5)
    rois = []
    for r in morph_cases.shapes() + morph_cases.ring():
        p = rng.permutation(len(r["x"]))
        rois.append(dict(r, x=r["x"][p], y=r["y"][p], inten=np.asarray(r["inten"])[p]))
    want = np.vstack([rows(hip_ctx, "shapes"), rows(hip_ctx, "ring")])
    assert same(hip_ctx.morph_host(_abi.batch_from_rois(rois), ALL, s), want)


def test_placed(hip_ctx):
    got, k = rows(hip_ctx, "placed"), morph_cases.N_PLACED
    c = {n: i for i, n in enumerate(N)}
    free = [c[n] for n in N if n not in morph_ref.POSITION and n not in morph_ref.CENTROID_BOUND]
    for p, (ox, oy) in enumerate(morph_cases.PLACEMENTS):
        blk = got[p * k:(p + 1) * k]
        assert same(blk[:, free], got[:k, free]), p                          # position-free columns keep their bits
        for n in morph_ref.EXTREMA + ["BBOX_XMIN", "BBOX_YMIN"]:             # position columns move by the origin exactly
            assert (blk[:, c[n]] - got[:k, c[n]] == (ox if n in morph_ref.POSITION_X else oy)).all(), (p, n)
        for n in morph_ref.CENTROID_BOUND:
            assert (np.abs(blk[:, c[n]] - got[:k, c[n]]) <= morph_ref.CENTROID_ULPS * np.spacing(float(max(ox, oy, 1)))).all(), (p, n)


def test_origins_null_equals_origins_of_zeros(hip_ctx):
    s = _abi.default_settings(64)
    b = morph_cases.batch("shapes")
    assert b.origin_x is not None and not np.asarray(b.origin_x).any() and not np.asarray(b.origin_y).any()
    plain = _abi.HostBatch(b.roi_label, b.px_offset, b.x, b.y, b.inten, b.bbox_w, b.bbox_h, b.min_inten, b.max_inten)
    assert plain.origin_x is None and same(hip_ctx.morph_host(plain, ALL, s), rows(hip_ctx, "shapes"))
    k = morph_cases.N_PLACED
    assert same(_device_rows(hip_ctx, morph_cases.batch("placed"), ALL, True, origins=False), np.tile(rows(hip_ctx, "placed")[:k], (4, 1)))


def test_tile_entry(hip_ctx):
    it, lab = morph_cases.tile()
    b = morph_cases.batch("tile")
    s = _abi.default_settings(64)
    want = rows(hip_ctx, "tile")
    for m in (ALL, _abi.MORPH_CONTOUR, _abi.MORPH_BASIC | _abi.MORPH_EXTREMA):
        tiles, labels, T = hip_ctx.morph_tiles_host(it[None], lab[None], m, s)
        assert list(labels) == list(b.roi_label) and list(tiles) == [0] * b.n_roi and same(T, want[:, morph_ref.columns_of(m)]), m
    tiles, labels, T = hip_ctx.morph_tiles_host(np.stack([it] * 3), np.stack([lab] * 3), ALL, s, max_device_bytes=1 << 20)
    assert list(tiles) == [0] * b.n_roi + [1] * b.n_roi + [2] * b.n_roi and list(labels) == list(b.roi_label) * 3 and same(T, np.tile(want, (3, 1)))
    ft, fl, _ = hip_ctx.featurize_tiles_host(it[None], lab[None], _abi.FAM_EULER, s)     # the row order of nyxhip_featurize_tiles_v2
    assert list(fl) == list(labels[:b.n_roi]) and list(ft) == [0] * b.n_roi


def test_through_nyxus_morphology_featurize():
    api = json.load(open(os.path.join(ROOT, "tests", "golden", "morph", "api_expected.json")))
    it, lab = morph_cases.tile()
    for key in ("five_codes", "basic_group", "all_41"):
        case = api["cases"][key]
        df = nyxus_amd.NyxusMorphology(case["features"]).featurize(it.astype(api["inten_dtype"]), lab)
        assert list(df.columns[4:]) == case["columns"] and list(df["ROI_label"]) == api["labels"], key
        got, want = df[case["columns"]].values.astype(float), np.array(case["numeric"])
        assert np.isfinite(got).all() and (np.abs(got - want) <= parity.REL_TOL * np.abs(want)).all(), key
    case = api["cases"]["mixed"]                                             # morphology codes beside codes of class Nyxus, in enum order
    df = nyxus_amd.NyxusMorphology(case["features"]).featurize(it.astype(api["inten_dtype"]), lab)
    cols = list(df.columns[4:])
    assert case["order"][-1] == "GLCM_ASM" and cols == case["order"][:-1] + ["GLCM_ASM_%d" % a for a in (0, 45, 90, 135)]
    got, want = df[case["columns"]].values.astype(float), np.array(case["numeric"])
    assert (np.abs(got - want) <= parity.REL_TOL * np.abs(want)).all()
    others = [c for c in cols if c not in N]
    plain = nyxus_amd.Nyxus([f for f in case["features"] if f not in N]).featurize(it.astype(api["inten_dtype"]), lab)
    assert list(plain.columns[4:]) == others and same(plain[others].values.astype(float), df[others].values.astype(float))
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["PERIMETER"])


def test_soft_nan_reaches_the_table_only_through_finalisation(hip_ctx):
    s = _abi.default_settings(64)
    s.soft_nan = -7.5
    for name in ("small", "shapes"):
        assert same(hip_ctx.morph_host(morph_cases.batch(name), ALL, s), rows(hip_ctx, name)), name      # raw: +inf stays
    raw = rows(hip_ctx, "small").copy()
    assert np.isinf(raw).sum() == 3 and not (raw == -7.5).any()
    _lib.load().nyxhip_finalize_table(raw.ctypes.data, raw.shape[0], raw.shape[1], raw.shape[1], __import__("ctypes").c_double(-7.5))
    assert np.isfinite(raw).all() and (raw == -7.5).sum() == 3 and (raw[:, N.index("CIRCULARITY")] == -7.5).tolist() == [True, True, False, False, False, True]


def test_argument_errors(hip_ctx):
    import ctypes as C
    lib, s = _lib.load(), _abi.default_settings(64)
    b = morph_cases.batch("small")
    for m in (0, 16, 0x1F, 1 << 31):
        with pytest.raises(_lib.NyxHipError) as ei:
            hip_ctx.morph_host(b, m, s)
        assert ei.value.code == 1
    cb = b.c_struct()
    out = np.zeros((b.n_roi, 41))
    call = lambda batch, ox, oy, m, st, o, ld: lib.nyxhip_morph_batch(hip_ctx._h, batch, ox, oy, m, st, o, ld)   # noqa: E731
    ox = np.zeros(b.n_roi, np.uint32)
    assert call(C.byref(cb), ox.ctypes.data, None, ALL, C.byref(s), out.ctypes.data, 41) == 1              # one origin NULL
    assert call(C.byref(cb), None, ox.ctypes.data, ALL, C.byref(s), out.ctypes.data, 41) == 1
    assert call(C.byref(cb), None, None, ALL, C.byref(s), out.ctypes.data, 40) == 1                        # ld too small
    assert call(C.byref(cb), None, None, _abi.MORPH_HULL, C.byref(s), out.ctypes.data, 2) == 1
    assert call(None, None, None, ALL, C.byref(s), out.ctypes.data, 41) == 1                               # null batch / settings / table
    assert call(C.byref(cb), None, None, ALL, None, out.ctypes.data, 41) == 1
    assert call(C.byref(cb), None, None, ALL, C.byref(s), None, 41) == 1
    for field in ("px_offset", "x", "y", "inten", "bbox_w", "bbox_h"):                                    # null arrays
        bad = b.c_struct()
        setattr(bad, field, None)
        assert call(C.byref(bad), None, None, ALL, C.byref(s), out.ctypes.data, 41) == 1, field
    empty = b.c_struct()
    empty.n_roi = 0
    assert call(C.byref(empty), None, None, ALL, C.byref(s), out.ctypes.data, 41) == 0                     # an empty batch is OK
    assert call(C.byref(cb), None, None, ALL, C.byref(s), out.ctypes.data, 41) == 0 and same(out, rows(hip_ctx, "small"))
    it, lab = morph_cases.tile()
    with pytest.raises(_lib.NyxHipError) as ei:
        hip_ctx.morph_tiles_host(it[None], lab[None], 16, s)
    assert ei.value.code == 1
