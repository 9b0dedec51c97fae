"""The neighbor columns on the GPU (nyxhip_neighbors_batch / nyxhip_neighbors_tiles): the HIP rows against values recorded from the
reference's own class (tests/golden/neighbors), and against themselves across every way a row can be requested.

Tolerances against the recorded values:
  equal bits        NUM_NEIGHBORS, PERCENT_TOUCHING, CLOSEST_NEIGHBOR1_DIST, CLOSEST_NEIGHBOR2_DIST, ANG_BW_NEIGHBORS_MODE: their chain is
                    integers, IEEE operations and correctly rounded roots
  parity.REL_TOL    CLOSEST_NEIGHBOR1_ANG, CLOSEST_NEIGHBOR2_ANG, ANG_BW_NEIGHBORS_MEAN, ANG_BW_NEIGHBORS_STDDEV: the device's atan2 is
                    not libm's (the project's standing bound)."""
import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import neighbors_cases as nc, neighbors_ref as nr, parity

pytestmark = pytest.mark.gpu

GOLD = nc.golden()
EXACT_COLS = [i for i, n in enumerate(nr.NAMES) if n in nr.EXACT]
TOL_COLS = [i for i, n in enumerate(nr.NAMES) if n not in nr.EXACT]
_ROWS = {}


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def rows(ctx, name, radius):
    """The nine columns of a case through the batch entry, computed once and shared."""
    if (name, radius) not in _ROWS:
        _ROWS[(name, radius)] = ctx.neighbors_host(nc.batch(name), radius, _abi.default_settings(64))
    return _ROWS[(name, radius)]


@pytest.mark.parametrize("name,radius", nc.keys())
def test_hip_rows_match_the_reference_class(hip_ctx, name, radius):
    want = GOLD[(name, radius)][:, :9]
    got = rows(hip_ctx, name, radius)
    assert got.shape == want.shape and np.isfinite(got).all()
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print(f"{name} R={radius}: {len(got)} ROIs; largest relative difference per column {dict(zip(nr.NAMES, rel.max(0)))}")
    bad = np.argwhere(got[:, EXACT_COLS] != want[:, EXACT_COLS])
    assert not len(bad), [(r, nr.NAMES[EXACT_COLS[c]], got[r, EXACT_COLS[c]], want[r, EXACT_COLS[c]]) for r, c in bad[:8]]
    g, w = got[:, TOL_COLS], want[:, TOL_COLS]
    bad = np.argwhere(~(np.abs(g - w) <= parity.REL_TOL * np.abs(w)))
    assert not len(bad), [(r, nr.NAMES[TOL_COLS[c]], g[r, c], w[r, c]) for r, c in bad[:8]]


def test_rows_are_repeatable(hip_ctx):
    s = _abi.default_settings(64)
    for name, radius in (("contacts", 2), ("lattice", 12), ("long_comb", 5), ("three_images", 5)):
        assert same(hip_ctx.neighbors_host(nc.batch(name), radius, s), rows(hip_ctx, name, radius)), name


def test_each_image_alone_gives_its_rows_of_the_multi_image_call(hip_ctx):
    s = _abi.default_settings(64)
    for name, radius in (("three_images", 5), ("three_images", 12), ("words", 5)):
        labs = nc.images(name)
        full = rows(hip_ctx, name, radius)
        b = nc.batch(name)
        for k, (lo, hi) in enumerate(nr.image_ranges(b)):
            alone = hip_ctx.neighbors_host(nc.batch_of_images(labs[k:k + 1], seed0=500 + k), radius, s)
            assert same(alone, full[lo:hi]), (name, k)
    # identical geometry under other labels: identical rows -- and no neighbor across images (the same boxes, image after image)
    T = rows(hip_ctx, "three_images", 12)
    assert same(T[:16], T[16:32]) and same(T[:16], T[32:])
    # image_offset None: one image
    one = nc.batch("contacts")
    one.image_offset = None
    assert same(hip_ctx.neighbors_host(one, 5, s), rows(hip_ctx, "contacts", 5))


@pytest.mark.parametrize("name", [n for n, c in nc.CASES.items() if c[2] is None])
def test_tile_entry_gives_the_bits_of_the_batch_entry(hip_ctx, name):
    s = _abi.default_settings(64)
    I, M = nc.stack(name)
    b = nc.batch(name)
    for radius in nc.CASES[name][1]:
        tiles, labels, table = hip_ctx.neighbors_tiles_host(I, M, radius, s)
        assert labels.tolist() == np.asarray(b.roi_label).tolist()
        assert tiles.tolist() == np.repeat(np.arange(len(M)), np.diff(b.image_offset.astype(np.int64))).tolist()
        assert same(table, rows(hip_ctx, name, radius)), (name, radius)
    if len(M) > 1:                                                           # a budget of a tile or two: the stack in several chunks
        tiles, labels, table = hip_ctx.neighbors_tiles_host(I, M, nc.CASES[name][1][0], s, max_device_bytes=400_000)
        assert same(table, rows(hip_ctx, name, nc.CASES[name][1][0]))


def test_origins_against_both_null(hip_ctx):
    """An image whose ROIs' boxes all start at (0, 0) -- a block in the corner and a hook around it: with the origins and with both
    NULL the same bits.  Moving every origin by the same amount keeps the integer columns and the distances."""
    s = _abi.default_settings(64)
    lab = np.zeros((16, 16), np.uint32)
    lab[0:3, 0:3] = 1
    lab[0:2, 6:14] = 2; lab[0:14, 12:14] = 2; lab[12:14, 0:14] = 2           # the hook: its box starts at (0, 0) as well
    b = nc.batch_of_images([lab])
    assert np.asarray(b.origin_x).tolist() == [0, 0] and np.asarray(b.origin_y).tolist() == [0, 0]
    with_o = hip_ctx.neighbors_host(b, 5, s)
    b0 = nc.batch_of_images([lab])
    b0.origin_x = b0.origin_y = None
    assert same(hip_ctx.neighbors_host(b0, 5, s), with_o)
    want = nr.table(b, 5)[:, :9]
    assert (with_o[:, EXACT_COLS] == want[:, EXACT_COLS]).all() and with_o[0, 0] == 1
    assert (np.abs(with_o - want) <= parity.REL_TOL * np.abs(want)).all()
    placed, base = rows(hip_ctx, "placed", 5), rows(hip_ctx, "contacts", 5)
    assert same(placed[:, [0, 1, 2, 4, 8]], base[:, [0, 1, 2, 4, 8]])        # (centroid differences of these boxes are exact beyond 2^24 too)


def test_errors(hip_ctx):
    s = _abi.default_settings(64)
    b = nc.batch("contacts")
    good = rows(hip_ctx, "contacts", 5)
    for bad_distance in (0, -3):
        with pytest.raises(_lib.NyxHipError) as ei:
            hip_ctx.neighbors_host(b, bad_distance, s)
        assert ei.value.code == 1
    with pytest.raises(_lib.NyxHipError) as ei:
        hip_ctx.neighbors_tiles_host(*nc.stack("contacts"), 0, s)
    assert ei.value.code == 1
    d = nc.batch("contacts")
    lab = np.asarray(d.roi_label).copy()
    lab[[3, 4]] = lab[[4, 3]]                                                # descending labels inside an image
    d.roi_label = lab
    with pytest.raises(_lib.NyxHipError) as ei:
        hip_ctx.neighbors_host(d, 5, s)
    assert ei.value.code == 1
    assert same(hip_ctx.neighbors_host(b, 5, s), good)                       # the context serves the next call


def test_through_nyxus_featurize(hip_ctx):
    api = nc.api_expected()
    I, M = nc.stack(api["case"])
    want = {int(r): np.asarray(t) for r, t in api["numeric"].items()}
    frames = {}
    for radius in (2, 5):
        nyx = nyxus_amd.Nyxus(["*ALL_NEIGHBOR*"], neighbor_distance=radius)
        df = nyx.featurize(I, M)
        assert list(df.columns[4:]) == api["columns"] and df["ROI_label"].tolist() == api["labels"]
        got = df[api["columns"]].to_numpy()
        assert (got[:, EXACT_COLS] == want[radius][:, EXACT_COLS]).all()
        assert (np.abs(got - want[radius]) <= parity.REL_TOL * np.abs(want[radius])).all()
        frames[radius] = got
    assert (frames[2] != frames[5]).any()                                    # neighbor_distance takes effect
    nyx = nyxus_amd.Nyxus(["NUM_NEIGHBORS"], neighbor_distance=2)
    nyx.set_environment_params(neighbor_distance=5)
    assert (nyx.featurize(I, M)["NUM_NEIGHBORS"].to_numpy() == want[5][:, 0]).all()
    # beside families: the nine columns sit behind EULER_NUMBER and in front of GLCM_ASM, the family columns are those of a call without them
    feats = ["MEAN", "GLCM_ASM", "EULER_NUMBER"]
    both = nyxus_amd.Nyxus(feats + ["*ALL_NEIGHBOR*"], neighbor_distance=5).featurize(I, M)
    fam = nyxus_amd.Nyxus(feats, neighbor_distance=5).featurize(I, M)
    assert list(both.columns[4:6]) == ["MEAN", "EULER_NUMBER"] and list(both.columns[6:15]) == api["columns"] and both.columns[15] == "GLCM_ASM_0"
    assert same(both[list(fam.columns[4:])].to_numpy(), fam[list(fam.columns[4:])].to_numpy())
    assert same(both[api["columns"]].to_numpy(), frames[5])
    assert both["ROI_label"].tolist() == api["labels"]


def test_family_calls_around_a_neighbor_call_keep_their_bits(hip_ctx):
    """The contour workspace is shared: a family call before and after a neighbors call on the same context returns identical bits."""
    s = _abi.default_settings(64)
    mask = _abi.FAM_CIRCLES | _abi.FAM_GEODETIC | _abi.FAM_ROI_RADIUS | _abi.FAM_SMOMS
    b = nc.batch("ring")
    before = hip_ctx.featurize_host(b, mask, s)
    nb = hip_ctx.neighbors_host(b, 5, s)
    after = hip_ctx.featurize_host(b, mask, s)
    assert same(before, after) and same(nb, rows(hip_ctx, "ring", 5))
