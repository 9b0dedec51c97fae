"""GPU test of the builds of the metric kernel (nyxus_amd/csrc/features_plan.h: NYX_FEATURE_BUILDS, plan_features_launch) that a batch
reaches only when its carve-out happens to land there: the occupancy tiers 4 .. 7 of the cloud and the window loader (NYXHIP_MAX_OCC, a
per-call knob, caps the tier), the generic (C16, SPLIT, D8) sets, and the two builds for grey depths 17 .. 64.

Every call is held to the oracle (parity.compare_tables; the integer-sum columns exactly) AND to the build its launch line names
(NYXHIP_DEBUG: `... build tier T fam F win W c16 . split . d8 . nw N defer D`, tests/device_call.py::launch_builds) -- a batch that slid
to another build would pass the first check and test nothing new."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import device_call as dc
from tests import parity, synth
from tests.test_cloud_trips_gpu import _rois, _roi, BOX_H, INT_EXACT

pytestmark = pytest.mark.gpu

BOTH = _abi.FAM_INTENSITY | _abi.FAM_GLCM
MASKS = [BOTH, _abi.FAM_INTENSITY, _abi.FAM_GLCM]

_cache = {}


def _oracle(key, make):
    """(batch or None, settings, oracle table) per key: computed once, shared, never written to."""
    if key not in _cache:
        _cache[key] = make()
        _cache[key][-1].setflags(write=False)
    return _cache[key]


def _cloud_case(kind, gd, mask):
    def make():
        if kind == "range17":                                        # ranges beyond 16 bits: the fused kernel sorts (32-bit tables), class 3
            rng = np.random.default_rng(7)
            rois = [_roi(n, BOX_H, rng.integers(1, 200001, n)) for n in (300, 1025, 2821)]
        elif kind == "box30":                                        # 30 x 30 boxes: below the eight-wave box of the grey-depth-64 launch
            rng = np.random.default_rng(8)
            rois = [_roi(n, 30, rng.integers(1, 4096, n)) for n in (257, 600, 899, 900)]
        else:
            rois = _rois(kind)
        b, s = _abi.batch_from_rois(rois), _abi.default_settings(gd)
        return b, s, po.oracle_featurize(b, mask, s)
    return _oracle((kind, gd, mask), make)


def _check(G, O, names, b=None):
    bad = parity.compare_tables(G, O, names, batch=b)
    assert not bad, "\n".join(bad[:20])
    for c in INT_EXACT:                                               # sums of integers: no rounding to allow for
        if c in names:
            j = names.index(c)
            assert np.array_equal(G[:, j], O[:, j]), (c, np.nonzero(G[:, j] != O[:, j])[0][:10])


def _builds(err, mask=None):
    """The body builds the launch lines of a call name (the wave-per-ROI kernel's lines left out; with `mask`, only the launches of
    that family set); at least one."""
    lines, builds = dc.launch_lines(err), dc.launch_builds(err)
    assert len(builds) == len(lines), err[-2000:]
    body = [b for l, b in zip(lines, builds) if b != "small" and (mask is None or l[4] == mask)]
    assert body, err[-2000:]
    return body


def _call(ctx, b, mask, s, capfd):
    """One call on stated extrema -> (table, the stderr of that call alone: the priming call's launch lines are dropped)."""
    dc.prime_census(ctx, mask, s)
    capfd.readouterr()
    G, rep = dc.device_call(ctx, b, mask, s, stated=True, prime=False)
    return G, capfd.readouterr().err, rep


def _set_occ(monkeypatch, occ):
    monkeypatch.setenv("NYXHIP_DEBUG", "1")
    if occ is None:
        monkeypatch.delenv("NYXHIP_MAX_OCC", raising=False)
    else:
        monkeypatch.setenv("NYXHIP_MAX_OCC", str(occ))


def _assert_tier(body, mask, occ, win):
    tier = min(8, occ or 8)
    for b in body:
        assert (b["tier"], b["win"], b["nw"]) == (tier, win if tier >= 6 else 2, 4), body
        assert b["fam"] == (dc.COMPACT_FAM[mask] if tier >= 6 else 0), body         # the compile-time family sets: tiers 8, 7, 6
        assert b["defer"] == int(tier == 8 and bool(mask & _abi.FAM_INTENSITY)), body


@pytest.mark.parametrize("occ", [4, 5, 6, 7])
@pytest.mark.parametrize("mask", MASKS)
def test_cloud_tiers(hip_ctx, mask, occ, monkeypatch, capfd):
    """The trip-boundary batch (held to the eight-per-CU carve-out) under every occupancy cap."""
    b, s, O = _cloud_case("tiny_nz", 8, mask)
    _set_occ(monkeypatch, occ)
    G, err, rep = _call(hip_ctx, b, mask, s, capfd)
    assert all(r["class"] < 0 for r in rep), rep                      # whole-batch launches, nothing counted
    assert max(l[3] for l in dc.launch_lines(err)) <= dc.OCC8_LDS, err[-2000:]
    _assert_tier(_builds(err), mask, occ, win=0)
    _check(G, O, _lib.column_names(mask, s), b)


def _tile_case(mask):
    def make():
        rng = np.random.default_rng(51)
        lab = synth.disk_label_tile(size=256, pitch=64, radius=25).astype(np.uint32)
        inten = rng.integers(1, 4096, (2, 256, 256)).astype(np.uint32)
        s = _abi.default_settings(8)
        rows = [po.oracle_featurize(_abi.batch_from_rois(synth.rois_from_tile(inten[t], lab)), mask, s) for t in range(2)]
        return inten, np.stack([lab, lab]), s, np.concatenate(rows)
    return _oracle(("tiles", mask), make)


@pytest.mark.parametrize("occ", [None, 7, 6])
@pytest.mark.parametrize("mask", MASKS)
def test_window_tiers(hip_ctx, mask, occ, monkeypatch, capfd):
    """Two tiles of 16 disks through the tile path: the window loader's builds at tiers 8, 7 and 6."""
    inten, lab, s, O = _tile_case(mask)
    _set_occ(monkeypatch, occ)
    tiles, labels, T = hip_ctx.featurize_tiles_host(inten, lab, mask, s)
    err = capfd.readouterr().err
    assert len(labels) == len(O) == 32
    _assert_tier(_builds(err), mask, occ, win=1)
    _check(T, O, _lib.column_names(mask, s))


# (value kind, grey depth, mask) -> the (C16, SPLIT, D8) set make_layout and build_args produce for it on a whole-batch launch:
#   grey depth 8, small ranges: the 16-bit tables, the split GLCM features, the 8-bit plane
#   grey depths -16 (radiomics binning) and 100: no split, 16-bit planes; the 16-bit tables with the intensity block ...
#   ... and no table at all without it
#   ranges beyond 16 bits at grey depth 8: 32-bit tables, 16-bit plane, the split (a class list of the fused sort kernel; the GLCM-only
#   launch beside it, for members of 16-bit range, is another family set's and is left out)
GENERIC = [("tiny_nz", 8, BOTH, (1, 1, 1)), ("tiny_nz", -16, BOTH, (1, 0, 0)), ("tiny_nz", 100, BOTH, (1, 0, 0)), ("tiny_nz", 100, _abi.FAM_GLCM, (0, 0, 0)),
           ("range17", 8, BOTH, (0, 1, 0))]


@pytest.mark.parametrize("occ", [4, None])
@pytest.mark.parametrize("kind,gd,mask,want", GENERIC, ids=lambda v: str(v).replace(" ", ""))
def test_generic_sets(hip_ctx, kind, gd, mask, want, occ, monkeypatch, capfd):
    b, s, O = _cloud_case(kind, gd, mask)
    _set_occ(monkeypatch, occ)
    G, err, rep = _call(hip_ctx, b, mask, s, capfd)
    body = _builds(err, mask)
    for bd in body:
        assert (bd["c16"], bd["split"], bd["d8"]) == want, body
        if occ == 4:
            assert (bd["tier"], bd["fam"], bd["win"], bd["defer"]) == (4, 0, 2, 0), body
    _check(G, O, _lib.column_names(mask, s), b)


@pytest.mark.parametrize("kind,nw", [("tiny_nz", 8), ("box30", 4)])
def test_grey_depth_64_waves(hip_ctx, kind, nw, monkeypatch, capfd):
    """GLCM alone at the reference's default grey depth: eight waves per ROI from a class box of 48 x 48 cells on, four below."""
    mask = _abi.FAM_GLCM
    b, s, O = _cloud_case(kind, 64, mask)
    assert ((b.bbox_w * b.bbox_h).max() >= 2304) == (nw == 8)
    _set_occ(monkeypatch, None)
    G, err, rep = _call(hip_ctx, b, mask, s, capfd)
    body = _builds(err)
    for bd in body:
        assert (bd["tier"], bd["nw"], bd["fam"], bd["win"]) == (9, nw, 4 if nw == 8 else 0, 0), body
    _check(G, O, _lib.column_names(mask, s), b)
