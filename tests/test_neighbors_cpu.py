"""The neighbor class (NUM_NEIGHBORS .. ANG_BW_NEIGHBORS_MODE; nyxhip_neighbors_batch / nyxhip_neighbors_tiles), the parts that need no
GPU: the entries and their column names, the catalogue of every family mask (unchanged: the class claims no family bit), the feature-set
plumbing, and tests/neighbors_ref.py against values recorded from the reference's own class (tests/golden/neighbors) -- all nine columns
of every ROI, bit for bit."""
import hashlib
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib, featureset
from tests import neighbors_cases as nc, neighbors_ref as nr

CI, GE = _abi.FAM_CIRCLES, _abi.FAM_GEODETIC
CAL = _abi.FAM_FERET | _abi.FAM_MARTIN | _abi.FAM_NASSENSTEIN
OUTLINE = _abi.FAM_FRACTAL | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS
EVERYTHING = _abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE | CAL | _abi.FAM_CHORDS | _abi.FAM_ELLIPSE | _abi.FAM_EROSION
# every mask tests/test_circle_cpu.py names
MASKS = [_abi.FAM_ALL, CAL, _abi.FAM_EULER, _abi.FAM_ROI_RADIUS, EVERYTHING, EVERYTHING | CI | GE, CI, GE, CI | GE,
         _abi.FAM_CHORDS | CI | GE | _abi.FAM_ROI_RADIUS | _abi.FAM_GLCM, CAL | _abi.FAM_INTENSITY | GE | _abi.FAM_GLCM,
         _abi.FAM_EULER | CI | _abi.FAM_ROI_RADIUS, _abi.FAM_INTENSITY | _abi.FAM_GLCM, OUTLINE, _abi.FAM_CHORDS,
         _abi.FAM_RADIAL | _abi.FAM_GABOR, _abi.FAM_EULER | _abi.FAM_CHORDS | _abi.FAM_ROI_RADIUS]
UNASSIGNED = (12, 14, 26, 27, 28, 29, 30, 31)
GOLD = nc.golden()


def test_entries_and_names():
    lib = _lib.load()
    for sym in ("nyxhip_neighbor_column_name", "nyxhip_neighbors_batch", "nyxhip_neighbors_tiles"):
        assert hasattr(lib, sym) and sym in _lib.ABI_SYMBOLS
    assert lib.nyxhip_abi_version() == 2
    assert _abi.NEIGHBOR_COLS == 9 == len(nr.NAMES)
    assert _lib.neighbor_column_names() == nr.NAMES == featureset.NEIGHBORS
    import ctypes as C
    buf = C.create_string_buffer(64)
    assert lib.nyxhip_neighbor_column_name(-1, buf, 64) == 1 and lib.nyxhip_neighbor_column_name(9, buf, 64) == 1
    assert lib.nyxhip_neighbor_column_name(0, None, 64) == 1
    assert hasattr(_lib.Context, "neighbors_host") and hasattr(_lib.Context, "neighbors_tiles_host")


def test_family_catalogue_is_unchanged():
    """The class claims no family bit: every mask keeps its columns (count and SHA-256 of the names, recorded from the commit before the
    neighbor entries: family_columns.json), the unassigned bits stay out, no column carries a neighbor name."""
    s = _abi.default_settings(64)
    lib = _lib.load()
    want = json.load(open(os.path.join(nc.GOLDEN_DIR, "family_columns.json")))
    for m in MASKS:
        names = _lib.column_names(m, s)
        assert lib.nyxhip_n_columns(m, s) == len(names)
        assert [len(names), hashlib.sha256("\n".join(names).encode()).hexdigest()] == want[str(m)], hex(m)
        assert not set(names) & set(nr.NAMES)
    for bit in UNASSIGNED:
        assert _lib.column_names(1 << bit, s) == []
    assert featureset.FAM_NEIGHBORS == 1 << 32 and not featureset.FAM_NEIGHBORS & 0xFFFFFFFF


def test_expand_marker_and_order():
    N = featureset.NEIGHBORS
    assert featureset.expand(["*ALL_NEIGHBOR*"]) == (featureset.FAM_NEIGHBORS, N)
    assert featureset.GROUPS["*ALL_NEIGHBOR*"] == N
    for code in N:
        assert featureset.FAMILY_OF[code] == featureset.FAM_NEIGHBORS
        assert featureset.expand([code.lower()]) == (featureset.FAM_NEIGHBORS, [code])
    assert featureset.expand(["ANG_BW_NEIGHBORS_MODE", "NUM_NEIGHBORS", "CLOSEST_NEIGHBOR2_ANG"])[1] == ["NUM_NEIGHBORS", "CLOSEST_NEIGHBOR2_ANG", "ANG_BW_NEIGHBORS_MODE"]
    assert featureset.split_neighbors(featureset.FAM_NEIGHBORS | _abi.FAM_GLCM) == (_abi.FAM_GLCM, True)
    assert featureset.split_neighbors(_abi.FAM_ALL) == (_abi.FAM_ALL, False)
    mask, order = featureset.expand(["GLCM_ASM", "PERCENT_TOUCHING", "ROI_RADIUS_MEDIAN", "MEAN", "NUM_NEIGHBORS", "EULER_NUMBER"])
    assert mask == featureset.FAM_NEIGHBORS | _abi.FAM_GLCM | _abi.FAM_ROI_RADIUS | _abi.FAM_INTENSITY | _abi.FAM_EULER
    assert order == ["MEAN", "EULER_NUMBER", "ROI_RADIUS_MEDIAN", "NUM_NEIGHBORS", "PERCENT_TOUCHING", "GLCM_ASM"]
    # behind ROI_RADIUS_*, in front of GLCM_*; the six older lists keep the codes they had
    R = featureset.REQUEST_ORDER
    k = R.index("ROI_RADIUS_MEDIAN")
    assert R[k + 1:k + 10] == N and R[k + 10] == "GLCM_ASM"
    assert [n for n in R if n not in N] == featureset.EXPAND_ORDER
    for frozen in (featureset.ENUM_ORDER, featureset.OUTPUT_ORDER, featureset.SERVED_ORDER, featureset.CATALOGUE_ORDER, featureset.FULL_ORDER,
                   featureset.EXPAND_ORDER):
        assert not set(N) & set(frozen)
    # the column selector over the family table with the nine columns to its right
    s = _abi.default_settings(64)
    fam, nb = featureset.split_neighbors(mask)
    names = _lib.column_names(fam, s) + _lib.neighbor_column_names()
    sel = featureset.column_selector(order, names, [0, 45, 90, 135])
    assert [names[j] for j in sel][:5] == order[:5] and names[sel[5]] == "GLCM_ASM_0"


def test_pinned_names_are_still_refused():
    for unserved in ("PERIMETER", "CIRCULARITY", "EDGE_MEAN_INTENSITY", "CONVEX_HULL_AREA", "AREA_PIXELS_COUNT", "EXTREMA_P1_X"):
        with pytest.raises(ValueError, match="not served by the MI355X path") as ei:
            featureset.expand([unserved])
        assert all(n in str(ei.value) for n in nr.NAMES) and "*ALL_NEIGHBOR*" in str(ei.value)
    for out_of_scope in ("HEXAGONALITY_AVE", "POLYGONALITY_AVE"):
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            featureset.expand([out_of_scope])


def test_nyxus_constructs_and_takes_the_distance():
    nyx = nyxus_amd.Nyxus(["NUM_NEIGHBORS"], neighbor_distance=3)
    assert nyx._mask == 0 and nyx._neighbors and nyx.get_params("neighbor_distance") == {"neighbor_distance": 3}
    nyx.set_environment_params(neighbor_distance=7)
    assert nyx._env["neighbor_distance"] == 7
    nyx = nyxus_amd.Nyxus(["MEAN", "*ALL_NEIGHBOR*", "GLCM_ASM"])
    assert nyx._mask == _abi.FAM_INTENSITY | _abi.FAM_GLCM and nyx._neighbors
    assert nyx._requested == ["MEAN"] + nr.NAMES + ["GLCM_ASM"]
    nyx.set_environment_params(features=["MEAN"])
    assert nyx._mask == _abi.FAM_INTENSITY and not nyx._neighbors
    with pytest.raises(ValueError, match="Neighbor distance"):
        nyxus_amd.Nyxus(["NUM_NEIGHBORS"], neighbor_distance=0)


@pytest.mark.parametrize("name", list(nc.CASES))
def test_restatement_matches_the_reference_class(name):
    """All nine columns, the contour length and the centroid of every ROI at every recorded radius, bit for bit."""
    from tests.radial_ref import contours_of
    b = nc.batch(name)
    K = contours_of(b)
    for radius in nc.CASES[name][1]:
        g = GOLD[(name, radius)]
        T = nr.table(b, radius, K)
        assert T.shape == g.shape == (b.n_roi, 12) and np.isfinite(g).all()
        assert (T == g).all(), [(r, (nr.NAMES + nr.EXTRA)[c], T[r, c], g[r, c]) for r, c in np.argwhere(T != g)[:8]]


def _row(b, label, image=0):
    lo, hi = nr.image_ranges(b)[image]
    return lo + int(np.nonzero(np.asarray(b.roi_label[lo:hi]) == label)[0][0])


def test_named_branches_occur_in_the_recorded_data():
    C1, C2, C5 = GOLD[("contacts", 1)], GOLD[("contacts", 2)], GOLD[("contacts", 5)]
    b = nc.batch("contacts")
    r = lambda lab: _row(b, lab)
    assert (C5[r(90), :9] == 0).all()                                        # isolated: all zeros
    assert C1[r(11), 0] == 1 and C1[r(11), 1] == 31.25                       # edge contact (d = 1)
    assert C1[r(21), 0] == 0 and C1[r(21), 1] == 6.25                        # diagonal only at R = 1: touching but NOT a neighbor
    assert C2[r(21), 0] == 1                                                 # ... (d = 2) a neighbor at R = 2
    assert C2[r(31), 0] == 1 and C2[r(31), 1] == 0 and C1[r(31), 0] == 0     # a one-pixel gap (d = 4)
    assert C5[r(41), 0] == 1 and C5[r(51), 0] == 0                           # gap exactly R | R + 1: a candidate, not a neighbor
    st = nr.table(b, 5, with_stats=True)[1]
    assert st["candidates"] == 7 and int(C5[:, 0].sum()) == 2 * 6
    assert nr.table(b, 1, with_stats=True)[1]["touch_not_neighbor"] == 1
    T = GOLD[("tiny", 5)]
    assert T[:, 9].tolist() == [32, 0, 0, 0] and (T[:, :9] == 0).all()       # 1 px, 2 px, an anti-diagonal: the pairs are skipped on both sides
    st = nr.table(nc.batch("tiny"), 5, with_stats=True)[1]
    assert st["skipped_empty"] == st["candidates"] == 5
    st = nr.table(nc.batch("corner"), 2, with_stats=True)[1]
    assert st["multi_touch_points"] >= 1                                     # one contour point adjacent to two neighbors: counted once
    K = GOLD[("corner", 2)]
    assert K[0, 1] == 100.0 * 7 / 16
    ck = GOLD[("checker", 5)]
    assert ck[0, 9] == 72 and ck[0, 0] == 2 and ck[0, 1] > 0                 # the bridged checkerboard: several sub-contours merged into one list
    Ti, bt = GOLD[("ties", 5)], nc.batch("ties")
    five = _row(bt, 5)
    assert Ti[five, 0] == 3 and Ti[five, 2] == Ti[five, 4] == 8.0            # bit-equal distances: the lower label wins, then the next one
    assert Ti[five, 3] == 180.0 and Ti[five, 5] == 0.0 and Ti[five, 7] > 0
    for lab in (20, 21):
        assert Ti[_row(bt, lab), 2] == 0.0 and Ti[_row(bt, lab), 3] == 0.0 and Ti[_row(bt, lab), 0] == 1   # the same centroid
    R2, R12 = GOLD[("row4", 2)], GOLD[("row4", 12)]
    assert R2[0, 0] == 1 and R2[0, 4] == 0 and R2[0, 5] == 0                 # exactly 1 neighbor: CLOSEST_NEIGHBOR2 absent
    assert R2[1, 0] == 2 and R2[1, 4] == 4.0 and R2[1, 7] == 0.0             # exactly 2: present, the deviation still 0
    assert R12[0, 0] == 3 and R12[0, 7] == 0.0 and R12[1, 7] > 0             # three equal angles: exactly 0; otherwise non-zero
    W = GOLD[("words", 2)]
    assert sorted(W[:, 9].astype(int).tolist()) == [7, 20, 42, 63, 64, 65, 257]
    br = json.load(open(os.path.join(nc.GOLDEN_DIR, "branches.json")))
    assert GOLD[("long_comb", 5)][0, 9] == br["comb_contour"] == 2641 > 2048
    assert GOLD[("ring", 5)][4, 9] == br["ring_contour"] and (131 + 2) ** 2 > 16384
    assert br["lattice_max_candidates"] > 64
    T3 = GOLD[("three_images", 5)]
    assert (T3[:16] == T3[16:32]).all() and (T3[:16] == T3[32:]).all()
    lab = np.asarray(nc.batch("three_images").roi_label)
    assert lab[16] == 10 and lab[17] == 17 and lab[32] == 100001             # non-contiguous labels
    P = GOLD[("placed", 5)]
    assert (P[:, 10] == C5[:, 10] + nc.FAR_X).all() and nc.FAR_X > 2 ** 24
    # the two conditions that keep the device's atan2 out of a decision
    for g in GOLD.values():
        sd, mean = g[:, 7], g[:, 6]
        assert (sd[sd != 0] >= 1e-3 * np.abs(mean[sd != 0])).all()
        for col in (3, 5):
            a = g[:, col]
            assert not ((np.abs(a - np.floor(a) - 0.5) < 1e-6) & (a != np.rint(a))).any()
