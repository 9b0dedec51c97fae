"""GPU tests: degenerate ROIs under a soft_nan that is not 0.0, on every launch path of the twelve core families.

At the default soft_nan = 0.0 a kernel that wrote soft_nan, one that wrote a literal zero and one that never wrote the cell (into a
zeroed buffer) give the same table.  Here soft_nan is -7.5 (tests/soft_nan_cases.py) and every expectation is the CPU oracle, which
tests/test_soft_nan_cpu.py pins to the reference's classes at that value -- in particular the GLCM row of a ROI whose binned minimum
equals its binned maximum is 0.0, not soft_nan (glcm.cpp:27-95 undone by save_value, :210-215).  Each test asserts from the expected
table that the rows served by the path it is about hold soft_nan somewhere, so that the comparison says something."""
import ctypes as C

import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import counts, parity, roi_assembly
from tests import soft_nan_cases as sc

pytestmark = pytest.mark.gpu

SOFT_NAN = sc.SOFT_NAN
INT, GLCM, INT_GLCM = _abi.FAM_INTENSITY, _abi.FAM_GLCM, _abi.FAM_INTENSITY | _abi.FAM_GLCM
DBL_MAX = 1.7976931348623157e308
POISON = -12345.0


def same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def mismatches(G, W, names, b):
    return parity.compare_tables(G, W, names, batch=b) + counts.compare_counts(G, W, names) + counts.compare_tight(G, W, names)


def expect(b, mask, s, rows=None, prefix=None):
    """The oracle's table; asserts that it holds soft_nan in `rows` (default: all) within the columns starting with `prefix`."""
    names = _lib.column_names(mask, s)
    O = po.oracle_featurize(b, mask, s)
    sub = O if rows is None else O[rows]
    cols = [j for j, n in enumerate(names) if prefix is None or n.startswith(prefix)]
    assert (sub[:, cols] == SOFT_NAN).any(), "the expected rows hold no soft_nan: the case proves nothing"
    return names, O


def check(ctx, rois, mask, s, rows=None, prefix=None, ref=True):
    b = _abi.batch_from_rois(rois)
    names, O = expect(b, mask, s, rows, prefix)
    G = ctx.featurize_host(b, mask, s)
    bad = mismatches(G, O, names, b)
    assert not bad, "\n".join(bad[:20])
    if ref and po.have_ref():
        bad = mismatches(G, po.ref_featurize(b, mask, s, n_threads=2), names, b)
        assert not bad, "vs reference classes:\n" + "\n".join(bad[:20])
    return G, O, names, b


def recorded(group, cfg, keep=None):
    """The reference classes' table of the degenerate set as recorded by tests/test_soft_nan_cpu.py."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_classes", f"softnan_{group}_{cfg}_degenerate.npz")
    with np.load(path) as z:
        T = z["table"]
    return T if keep is None else T[keep]


def against_recorded(G, names, group, cfg, mask, s, keep=None):
    sub = _lib.column_names(mask, s)
    col = {n: j for j, n in enumerate(names)}
    R = recorded(group, cfg, keep)
    bad = parity.compare_tables(G[:, [col[n] for n in sub]], R, sub)
    assert not bad, "vs recorded reference table:\n" + "\n".join(bad[:20])


# ---- INTENSITY | GLCM -----------------------------------------------------------------------------------------------------------------
SMALL_KEEP = [i for i in range(16) if i != sc.ROW64]


@pytest.mark.parametrize("mask", [INT, GLCM, INT_GLCM])
@pytest.mark.parametrize("gd", [8, 3, 16, 64, 33, 17])
def test_wave_per_roi_kernel(hip_ctx, mask, gd):
    """The degenerate set without its 64 x 1 row: every ROI is of the smallest size class (roi_small.hip); 33 and 17 levels and 64 take
    the pairs path.  INTENSITY alone never writes soft_nan: its rows equal the rows at soft_nan = 0 bit for bit."""
    rois = [sc.degenerate_rois()[i] for i in SMALL_KEEP]
    s = sc.settings(gd)
    if mask == INT:
        b = _abi.batch_from_rois(rois)
        G = hip_ctx.featurize_host(b, mask, s)
        assert not (G == SOFT_NAN).any() and same(G, hip_ctx.featurize_host(b, mask, sc.settings(gd, soft_nan=0.0))).all()
        bad = parity.compare_tables(G, po.oracle_featurize(b, mask, s), _lib.column_names(mask, s), batch=b)
        assert not bad, "\n".join(bad[:20])
    else:
        G, O, names, b = check(hip_ctx, rois, mask, s, prefix="GLCM_")
        early = b.min_inten == b.max_inten
        g = [j for j, n in enumerate(names) if n.startswith("GLCM_")]
        assert early.any() and (G[early][:, g] == 0.0).all()                  # the early-out rows are zeros, not soft_nan
        if gd in (8, 64):
            against_recorded(G, names, "glcm", f"gd{gd}", GLCM, s, SMALL_KEEP)
    rep = hip_ctx.launch_report()
    assert all(r["class"] == -2 or r["size_class"] == 0 for r in rep), rep    # nobody beyond the smallest class


def workgroup_case(gd, ibsi_max=0, eight_wave=False):
    rois = sc.workgroup_rois(n_random=1 if ibsi_max else 4)      # (IBSI: a matrix as large as the ROI's largest intensity)
    if eight_wave:
        rois.append(sc.eight_wave_companion())
    if ibsi_max:
        rois = [dict(r, inten=(np.asarray(r["inten"], np.uint64) % (ibsi_max + 1)).astype(np.uint32)) for r in rois]
        rois[-1]["inten"][0] = ibsi_max
    return rois, sc.settings(gd, bool(ibsi_max))


WG = [pytest.param(8, 0, False, id="gd8-deferred-close"), pytest.param(16, 0, False, id="gd16")]
WG += [pytest.param(gd, 0, w8, id=f"gd{gd}-{'eight' if w8 else 'four'}-waves") for gd in (17, 33, 64) for w8 in (False, True)]
WG += [pytest.param(gd, 0, False, id=f"gd{gd}-in-kernel") for gd in (20, 32, 48, -8, -24)]
WG += [pytest.param(gd, 0, False, id=f"gd{gd}-workspace") for gd in (255, 256)]
WG += [pytest.param(64, 200, False, id="ibsi-max200"), pytest.param(64, 1000, False, id="ibsi-max1000")]


@pytest.mark.parametrize("gd,ibsi_max,eight_wave", WG)
def test_workgroup_kernels(hip_ctx, gd, ibsi_max, eight_wave):
    """The same kinds one size class up (roi_features.hip and, for the 130 x 3 strip, the classes behind it), at every grey depth at
    which the GLCM block takes another path."""
    rois, s = workgroup_case(gd, ibsi_max, eight_wave)
    head = np.arange(sc.N_WORKGROUP_DEGENERATE)
    G, O, names, b = check(hip_ctx, rois, INT_GLCM, s, rows=head, prefix="GLCM_")
    early = np.nonzero(b.min_inten == b.max_inten)[0]
    g = [j for j, n in enumerate(names) if n.startswith("GLCM_")]
    assert len(early) >= 5 and (G[early][:, g] == 0.0).all()
    n_px = np.diff(b.px_offset.astype(np.int64))
    assert not ((n_px <= 256) & (np.maximum(b.bbox_w, b.bbox_h) <= 32)).any()          # nobody for the wave-per-ROI kernel
    rep = hip_ctx.launch_report()
    assert sum(r["rois"] for r in rep if r["class"] >= 0) in (0, b.n_roi), rep
    if gd in (255, 256):
        assert all(r["workspace"] == 1 for r in rep if r["class"] >= 0) and any(r["class"] >= 0 for r in rep), rep


@pytest.mark.parametrize("mask", [GLCM, INT_GLCM])
@pytest.mark.parametrize("gd", [8, 64])
def test_exact_class_lists(hip_ctx, mask, gd):
    """A wide-range companion (range beyond 16 bits) makes the call take exact class lists; the two-value ROI {1, 2^32 - 1} is of the
    wide-range class itself."""
    rois = sc.workgroup_rois(n_random=2) + [sc.degenerate_rois()[i] for i in (0, 3, 4, 9, 12, 13, 15)] + [sc.wide_range_companion(), sc.two_value_extremes()]
    check(hip_ctx, rois, mask, sc.settings(gd), rows=np.arange(len(rois) - 2), prefix="GLCM_")
    rep = hip_ctx.launch_report()
    assert all(r["class"] >= 0 for r in rep) and sum(r["rois"] for r in rep) == len(rois), rep
    if mask & INT:
        assert any(r["wide_range"] == 1 for r in rep), rep


@pytest.mark.parametrize("gd", [8, 64, -16])
def test_beyond_lds(hip_ctx, gd):
    """Constant, blank, two-value and one-non-zero-pixel 300 x 280 boxes (roi_large.hip) beside small ROIs."""
    check(hip_ctx, sc.beyond_lds_rois(), INT_GLCM, sc.settings(gd), rows=sc.BEYOND_LDS_BOXES, prefix="GLCM_")
    rep = hip_ctx.launch_report()
    assert sum(r["rois"] for r in rep if r["size_class"] == 4) == len(sc.BEYOND_LDS_BOXES), rep


# ---- GLRLM | GLSZM | NGTDM --------------------------------------------------------------------------------------------------------------
BIG = {"workgroup": (sc.workgroup_rois, np.arange(sc.N_WORKGROUP_DEGENERATE)), "beyond-lds": (sc.beyond_lds_rois, np.array(sc.BEYOND_LDS_BOXES))}
PREFIX = {_abi.FAM_GLRLM: "GLRLM_", _abi.FAM_GLSZM: "GLSZM_", _abi.FAM_NGTDM: "NGTDM_", _abi.FAM_GLDZM: "GLDZM_", _abi.FAM_GLDM: "GLDM_",
          _abi.FAM_NGLDM: "NGLDM_"}


@pytest.mark.parametrize("fam", [_abi.FAM_GLRLM, _abi.FAM_GLSZM, _abi.FAM_NGTDM, sc.TEXTURE])
@pytest.mark.parametrize("gd", [8, -20, 300])
@pytest.mark.parametrize("which", ["workgroup", "beyond-lds"])
def test_texture_families(hip_ctx, which, gd, fam):
    """roi_texture.hip and roi_large_tex.hip; 300 levels keep the 16-bit plane; the carve-out depends on the family set, so every family
    also runs alone."""
    make, rows = BIG[which]
    G, O, names, b = check(hip_ctx, make(), fam, sc.settings(gd), rows=rows, prefix=PREFIX.get(fam))
    for f, p in PREFIX.items():
        if fam & f:
            cols = [j for j, n in enumerate(names) if n.startswith(p)]
            assert (O[rows][:, cols] == SOFT_NAN).any(), p


# ---- GLDZM | GLDM | NGLDM ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gd,ibsi", [(8, False), (64, False), (20, True)])
@pytest.mark.parametrize("which", ["workgroup", "beyond-lds"])
def test_dependence_families(hip_ctx, which, gd, ibsi, monkeypatch):
    """Byte planes (8 levels), 16-bit planes (64) and IBSI levels; the three feature tails side by side against one after the other
    (NYXHIP_DEP_SEQ=1), bit for bit."""
    make, rows = BIG[which]
    rois = make()
    if ibsi:
        rois = sc.for_ibsi(rois, drop_blank=False)
    s = sc.settings(gd, ibsi)
    G, O, names, b = check(hip_ctx, rois, sc.DEPENDENCE, s, rows=rows)
    for p in ("GLDZM_", "GLDM_", "NGLDM_"):
        cols = [j for j, n in enumerate(names) if n.startswith(p)]
        assert (O[rows][:, cols] == SOFT_NAN).any(), p
    monkeypatch.setenv("NYXHIP_DEP_SEQ", "1")
    seq = hip_ctx.featurize_host(b, sc.DEPENDENCE, s)
    monkeypatch.delenv("NYXHIP_DEP_SEQ")
    assert np.array_equal(G.view(np.uint64), seq.view(np.uint64))


# ---- GABOR | ZERNIKE --------------------------------------------------------------------------------------------------------------------
def bank8(s):
    s.gabor_n_filters = 8
    for i in range(8):
        s.gabor_f0[i] = [4.0, 16.0, 32.0, 64.0][i % 4]
        s.gabor_theta[i] = np.pi * i / 8
    return s


def kersize(n):
    def f(s):
        s.gabor_kersize = n
        return s
    return f


@pytest.mark.parametrize("bank", [pytest.param(lambda s: s, id="default-bank"), pytest.param(bank8, id="bank8"), pytest.param(kersize(9), id="kernel9"),
                                  pytest.param(kersize(20), id="kernel20")])
@pytest.mark.parametrize("which", ["workgroup", "beyond-lds"])
def test_gabor_zernike(hip_ctx, which, bank):
    """roi_shape.hip and roi_large_gabor.hip: the default bank, eight orientations, and kernel sizes 9 and 20 (the generic kernel).
    Zernike of a constant ROI is soft_nan; Gabor of one is 0.0 (gabor.cpp:53-57) and stays bit-exact everywhere."""
    make, rows = BIG[which]
    s = bank(sc.settings(8))
    G, O, names, b = check(hip_ctx, make(), sc.SHAPE, s, rows=rows, prefix="ZERNIKE2D")
    gab = [j for j, n in enumerate(names) if n.startswith("GABOR")]
    assert len(gab) == s.gabor_n_filters and same(G[:, gab], O[:, gab]).all()
    early = b.min_inten == b.max_inten
    assert early.any() and (G[early][:, gab] == 0.0).all()


# ---- cross-family and call paths --------------------------------------------------------------------------------------------------------
def test_moments_and_intensity_never_write_soft_nan(hip_ctx):
    """Rows at soft_nan = -7.5 equal the rows at 0.0 bit for bit, raw NaN stays NaN; nyxhip_finalize_table then turns exactly the
    NaN / inf cells into soft_nan."""
    mask = sc.MOMENTS | sc.INTENSITY
    rois = sc.workgroup_rois(n_random=2) + sc.degenerate_rois()
    b = _abi.batch_from_rois(rois)
    s, s0 = sc.settings(8), sc.settings(8, soft_nan=0.0)
    names = _lib.column_names(mask, s)
    G, G0 = hip_ctx.featurize_host(b, mask, s), hip_ctx.featurize_host(b, mask, s0)
    assert same(G, G0).all()
    assert not (G == SOFT_NAN).any()
    O = po.oracle_featurize(b, mask, s)
    odd = np.argwhere(np.isnan(G) != np.isnan(O))
    assert np.isnan(O).any() and not len(odd), [(names[j], int(i), G[i, j], O[i, j]) for i, j in odd[:12]]
    bad = parity.compare_tables(G, O, names, batch=b)
    assert not bad, "\n".join(bad[:20])
    F = G.copy()
    _lib.load().nyxhip_finalize_table(F.ctypes.data, F.shape[0], F.shape[1], F.shape[1], C.c_double(SOFT_NAN))
    bad_cell = ~np.isfinite(G)
    assert bad_cell.any() and (F[bad_cell] == SOFT_NAN).all() and np.array_equal(F[~bad_cell], G[~bad_cell])


FAMILIES = [_abi.FAM_INTENSITY, _abi.FAM_GLCM, _abi.FAM_GLRLM, _abi.FAM_GLSZM, _abi.FAM_NGTDM, _abi.FAM_GABOR, _abi.FAM_ZERNIKE, _abi.FAM_GLDZM,
            _abi.FAM_GLDM, _abi.FAM_NGLDM, _abi.FAM_SMOMS, _abi.FAM_IMOMS]


def test_all_twelve_families_in_one_call(hip_ctx):
    """FAM_ALL over the workgroup set: every family's block equals the block of that family's call alone, bit for bit."""
    s = sc.settings(8)
    rois = sc.workgroup_rois(n_random=2)
    G, O, names, b = check(hip_ctx, rois, _abi.FAM_ALL, s, rows=np.arange(sc.N_WORKGROUP_DEGENERATE), ref=False)
    col = {n: j for j, n in enumerate(names)}
    assert len(col) == len(names)
    for fam in FAMILIES:
        sub = _lib.column_names(fam, s)
        alone = hip_ctx.featurize_host(b, fam, s)
        block = G[:, [col[n] for n in sub]]
        diff = np.argwhere(~same(alone, block))
        assert not len(diff), (hex(fam), [(sub[j], i, alone[i, j], block[i, j]) for i, j in diff[:6]])


def device_batch(b, dev):
    import torch
    keep = {k: torch.from_numpy(getattr(b, k).view({2: np.int16, 4: np.int32, 8: np.int64}[getattr(b, k).dtype.itemsize])).to(dev)
            for k in ("px_offset", "x", "y", "inten", "bbox_w", "bbox_h", "min_inten", "max_inten")}
    cb = b.c_struct()
    for k, t in keep.items():
        setattr(cb, k, t.data_ptr())
    cb.slide_min = None; cb.slide_max = None; cb.memory = _abi.MEM_DEVICE
    return cb, keep


@pytest.mark.parametrize("stated", [True, False])
@pytest.mark.parametrize("mask", [pytest.param(INT_GLCM, id="int-glcm"), pytest.param(sc.TEXTURE, id="texture"), pytest.param(_abi.FAM_ALL, id="all")])
def test_device_path_into_a_poisoned_table(hip_ctx, mask, stated):
    """featurize_device_async into a table with ld = ncol + 3 prefilled with a sentinel: every cell inside ncol is written, no cell of
    the padding is, and the table equals the host call's bit for bit -- on stated extrema and with the extrema left to the library."""
    import torch
    dev = torch.device("cuda", 0)
    rois = sc.workgroup_rois(n_random=2)[:7] + sc.degenerate_rois()[:7] + sc.degenerate_rois()[11:]      # (boxes <= 64: stated extrema keep whole-batch launches)
    b = _abi.batch_from_rois(rois)
    s = sc.settings(8)
    names, O = expect(b, mask, s)
    host = hip_ctx.featurize_host(b, mask, s)
    cb, keep = device_batch(b, dev)
    if not stated:
        cb.max_px = cb.max_bbox_area = cb.max_inten_range = cb.max_bbox_side = 0
    ncol = len(names)
    ld = ncol + 3
    out = torch.full((b.n_roi, ld), POISON, dtype=torch.float64, device=dev)
    hip_ctx.featurize_device_async(cb, mask, s, out.data_ptr(), ld)
    hip_ctx.sync()
    T = out.cpu().numpy()
    assert (T[:, ncol:] == POISON).all()
    unwritten = np.argwhere(T[:, :ncol] == POISON)
    assert not len(unwritten), [(names[j], i) for i, j in unwritten[:10]]
    diff = np.argwhere(~same(T[:, :ncol], host))
    assert not len(diff), [(names[j], i, T[i, j], host[i, j]) for i, j in diff[:10]]
    bad = mismatches(host, O, names, b)
    assert not bad, "\n".join(bad[:20])


def patch_tile(seed=0):
    """A 128 x 128 tile with a 4 x 4 grid of 24 x 24 labels on constant, blank, two-value, one-non-zero-pixel and random intensity
    patches, and a single-pixel label."""
    rng = np.random.default_rng(40 + seed)
    it = rng.integers(1, 4096, (128, 128)).astype(np.uint32)
    lab = np.zeros((128, 128), np.uint32)
    for k in range(16):
        y0, x0 = 32 * (k // 4) + 3, 32 * (k % 4) + 4
        lab[y0:y0 + 24, x0:x0 + 24] = 10 * (k + 1) + seed
        p = it[y0:y0 + 24, x0:x0 + 24]
        kind = (k + seed) % 5
        if kind == 0: p[:] = 1234
        elif kind == 1: p[:] = 0
        elif kind == 2: p[:] = np.where((np.arange(24)[:, None] + np.arange(24)[None, :]) % 2, 3000, 10)
        elif kind == 3: p[:] = 0; p[11, 7] = 77
    lab[30, 61] = 7                                     # a single-pixel label between the patches
    return it, lab


@pytest.mark.parametrize("mask", [pytest.param(INT_GLCM, id="window-mode"), pytest.param(INT_GLCM | _abi.FAM_NGTDM, id="cloud-mode")])
def test_tile_path(hip_ctx, mask):
    """featurize_tile_host and a stack of three through featurize_tiles_host under a 2 MiB device budget, against the batch path's rows
    of the same ROIs and against the oracle."""
    s = sc.settings(8)
    names = _lib.column_names(mask, s)
    tiles = [patch_tile(k) for k in range(3)]
    want = []
    for it, lab in tiles:
        b = roi_assembly.assemble(it, lab, DBL_MAX, -DBL_MAX)
        _, O = expect(b, mask, s, prefix="GLCM_")
        assert (O[:, [j for j, n in enumerate(names) if n.startswith("GLCM_")]] == 0.0).all(axis=1).any()
        want.append((b, O, hip_ctx.featurize_host(b, mask, s)))
    labels, T = hip_ctx.featurize_tile_host(tiles[0][0], tiles[0][1], mask, s)
    b, O, B = want[0]
    assert np.array_equal(labels, b.roi_label) and len(labels) == 17
    for W, what in ((B, "batch path"), (O, "oracle")):
        bad = mismatches(T, W, names, b)
        assert not bad, what + ":\n" + "\n".join(bad[:20])
    ti, labels, T = hip_ctx.featurize_tiles_host(np.stack([t[0] for t in tiles]), np.stack([t[1] for t in tiles]), mask, s, max_device_bytes=2 << 20)
    row = 0
    for k, (b, O, B) in enumerate(want):
        n = b.n_roi
        assert np.array_equal(labels[row:row + n], b.roi_label) and (ti[row:row + n] == k).all()
        for W, what in ((B, "batch path"), (O, "oracle")):
            bad = mismatches(T[row:row + n], W, names, b)
            assert not bad, f"tile {k}, {what}:\n" + "\n".join(bad[:20])
        row += n
    assert row == len(labels)
