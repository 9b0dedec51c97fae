"""ZERNIKE2D, the parts that need no GPU: the committed exact values (tests/golden/zernike) belong to the generators of
tests/zernike_cases.py and are reproduced by mpmath; the cases hold what they were built to hold (on-circle pixels in every category of
last-ulp and redo-band distance, a fused-multiply-add flip, the centre, the empty disc, every cloud size, every column above 1e-3); and the
reference's own algorithm -- the C oracle and, when built, the reference classes -- stays within the derived bound L(npx) of the exact value
on every case, which also proves that zernike_ref.members() restates the reference's in/out decision: one wrong decision moves a row by
thousands of units."""
import numpy as np
import pytest

from nyxus_amd import _abi
from oracle import pyoracle as po
from tests import zernike_cases as zc
from tests import zernike_ref as zr

GOLD = zc.golden()
ZE = _abi.FAM_ZERNIKE


def test_the_golden_file_belongs_to_the_generators():
    assert list(GOLD) == list(zc.CASES)
    for name in zc.CASES:
        roi = zc.roi(name)
        w, h = zc.box(roi)
        g = GOLD[name]
        assert g["hash"] == zr.input_hash(roi, w, h), name
        assert g["npx"] == len(roi["x"]) <= 9000, name
        assert g["kept"] == zc.members(roi)["n_kept"], name
        assert g["exact"].shape == (30,) and np.isfinite(g["exact"]).all() and (g["exact"] >= 0).all(), name


SAMPLE = ["edge_13_u8", "edge_13t_u32", "edge_13_u32_-4_-4_2", "edge_17t_u32_-4_-4_4", "centre_on_pixel_u32", "centre_r_below_1e-12",
          "centre_r_above_1e-12", "row_1x3", "col_257x1", "strip_2x65", "empty_disc", "l_shape", "ragged_2", "ragged_65", "ragged_257",
          "thin_33", "ring_half", "dumbbell", "dumbbell_skew"]


@pytest.mark.parametrize("name", SAMPLE)
def test_stored_values_are_reproduced_by_mpmath(name):
    got = zr.exact(zc.members(zc.roi(name)))
    assert [v.hex() for v in got] == [v.hex() for v in GOLD[name]["exact"]]
    if len(zc.roi(name)["x"]) <= 400:                                        # 50 digits are enough: 40 give the same values, far below a unit
        assert (np.abs(zr.exact(zc.members(zc.roi(name)), dps=40) - got) <= 1e-30).all()   # (moments that vanish by symmetry: 1e-40s)


def test_units_and_bound():
    assert zr.PAIRS[:4] == [(0, 0), (1, 1), (2, 0), (2, 2)] and zr.PAIRS[-5:] == [(9, 1), (9, 3), (9, 5), (9, 7), (9, 9)]
    assert zr.S(9, 1) == 681 and zr.S(8, 0) == 321 and zr.S(9, 9) == 1 and zr.S(0, 0) == 1
    assert [c for _, c in zr.coefficients(9, 1)] == [126, -280, 210, -60, 5]
    assert zr.unit(9, 1) == 2.0 ** -52 * 10 / np.pi * 681
    assert zr.bound(1) == 33 and zr.bound(256) == 33 and zr.bound(257) == 34 and zr.bound(8515) == 66


def test_every_sum_is_exact_in_double():
    for name in zc.CASES:
        mem = zc.members(zc.roi(name))
        assert 0 < mem["sum"] < 2 ** 53 and mem["m10"] < 2 ** 53 and mem["m01"] < 2 ** 53, name


def test_edge_bases_sit_on_the_circle():
    """Point symmetry: the centroid is the exact centre, and every lattice point with dx^2 + dy^2 = N^2 computes r2 = 1 or 1 + 2^-52 -- kept
    either way (sqrt rounds the latter to 1.0).  Both box orientations pick N."""
    for N in zc.EDGE_N:
        for tr in (False, True):
            offs = zc.edge_offsets(N, tr)
            assert len(offs) >= 6 and (N, 0) in offs + [(b, a) for a, b in offs]
            for mode in zc.MODES:
                roi = zc.roi(zc._edge_name(N, tr, mode))
                assert zc.box(roi) == ((N, 2 * N + 1) if tr else (2 * N + 1, N))
                mem = zc.members(roi)
                assert mem["m10"] * 2 == mem["sum"] * (zc.box(roi)[0] + 1) and mem["m01"] * 2 == mem["sum"] * (zc.box(roi)[1] + 1)
                top = int(roi["inten"].max())
                for _, k in zc.edge_pixels(roi, N, tr):
                    assert mem["r2"][k] in (1.0, 1.0 + 2.0 ** -52) and mem["r"][k] == 1.0 and mem["keep"][k], (N, tr, mode)
                    assert int(roi["inten"][k]) == top
                assert (roi["inten"] == top).sum() == len(offs)
    assert int(zc.roi("edge_65_u32")["inten"].max()) == 2 ** 32 - 1 and int(zc.roi("edge_65_u16")["inten"].max()) == 65535


def test_edge_cases_hold_every_category():
    """A condition on the committed set, not a measurement: at least 4 on-circle pixels in every category (the bands: on each side of 1), at
    least one whose decision a fused multiply-add turns, either way round."""
    have = {c: 0 for c in zc.CATEGORIES + zc.FLIPS}
    for name in zc.GROUPS["edge"]:
        N, tr = zc.edge_key(name)
        for c, n in zc.edge_census(zc.roi(name), N, tr).items():
            have[c] += n
    print("on-circle pixels per category:", have)
    for c in zc.CATEGORIES:
        assert have[c] >= 4, (c, have)
    for c in zc.FLIPS:
        assert have[c] >= 1, (c, have)
    for k in zc.EDGE_KEPT:
        assert zc._edge_name(*k) in zc.CASES
    assert {k[2] for k in zc.EDGE_KEPT} == {"u16", "u32"} and {k[1] for k in zc.EDGE_KEPT} == {False, True}


def test_centre_cases():
    r = {name: zc.centre_r(zc.roi(name)) for name in zc.GROUPS["centre"]}
    assert r["centre_on_pixel_u16"] == (0.0, False) and r["centre_on_pixel_u32"] == (0.0, False)     # r < DBL_EPSILON: dropped
    small = r["centre_smallest_r"]
    assert small[1] and zr.DBL_EPSILON <= small[0] < 1e-15                                            # kept, two ulps of 1 from the test
    assert all(small[0] < v[0] for k, v in r.items() if v[0] > 0 and k != "centre_smallest_r")
    assert r["centre_r_below_1e-12"][1] and 0.9e-12 < r["centre_r_below_1e-12"][0] < 1e-12            # the kernel's redo
    assert r["centre_r_above_1e-12"][1] and 1e-12 < r["centre_r_above_1e-12"][0] < 1.2e-12            # the kernel's fast path
    assert r["centre_r_fast_path"][1] and 1e-10 < r["centre_r_fast_path"][0] < 1e-9
    for name in zc.GROUPS["centre"]:                                         # the centre pixel is the brightest: its decision shows
        roi = zc.roi(name)
        c = zc.box(roi)[0] // 2
        assert roi["inten"][(roi["x"] == c) & (roi["y"] == c)][0] == roi["inten"].max()


def test_aspect_cases():
    for k in (2, 3, 64, 257):
        assert zc.box(zc.roi("row_1x%d" % k)) == (k, 1) and zc.box(zc.roi("col_%dx1" % k)) == (1, k)
        assert 1 <= GOLD["row_1x%d" % k]["kept"] <= 3 and 1 <= GOLD["col_%dx1" % k]["kept"] <= 3     # N = 1: the centroid's neighbours
    assert zc.box(zc.roi("strip_2x65")) == (65, 2) and zc.box(zc.roi("strip_65x2")) == (2, 65)
    assert GOLD["strip_2x65"]["kept"] < 12 and GOLD["strip_65x2"]["kept"] < 12                        # N = 2: most of the box is outside
    e = zc.roi("empty_disc")
    assert zc.box(e) == (12, 1) and e["inten"].min() != e["inten"].max()
    assert GOLD["empty_disc"]["kept"] == 0
    assert [v.hex() for v in GOLD["empty_disc"]["exact"]] == [0.0.hex()] * 30                         # thirty +0.0
    for name in ("l_shape", "ring_cloud"):
        w, h = zc.box(zc.roi(name))
        assert GOLD[name]["npx"] < w * h                                     # not a full rectangle


def _size_class(roi):
    """roi_class (nyxus_amd/csrc/roi_kernel.h): the first k with n_px <= kClassPx[k] and both sides <= kClassSide[k]."""
    n, side = len(roi["x"]), max(zc.box(roi))
    for k, (px, sd) in enumerate(zip((256, 4096, 16384, 32768), (32, 64, 128, 256))):
        if n <= px and side <= sd:
            return k
    return 4


def test_size_cases():
    assert [GOLD["ragged_%d" % n]["npx"] for n in zc.SIZES] == list(zc.SIZES)
    assert set(zc.SIZES) >= {2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 4099}
    for n in zc.SIZES:
        roi = zc.roi("ragged_%d" % n)
        assert len(set(zip(roi["x"].tolist(), roi["y"].tolist()))) == n      # a cloud: no pixel twice
        if n > 3:
            assert (roi["inten"] == 0).any() and zc.box(roi)[0] * zc.box(roi)[1] > n
    # the launch forms and the staging cap: a class-0 cloud (one wave alone), the same number of pixels in class 1 (four waves), and the
    # clouds around 4096 in ONE size class with their 5000-pixel companion, so that one launch stages 4096 and re-reads 4097
    assert _size_class(zc.roi(zc.CLASS0)) == 0 and all(_size_class(zc.roi("ragged_%d" % n)) == 0 for n in zc.SIZES if n <= 256)
    assert _size_class(zc.roi("thin_33")) == 1 and GOLD["thin_33"]["npx"] <= 256
    assert _size_class(zc.roi("companion_40x40")) == 1
    assert {_size_class(zc.roi(n)) for n in zc.CAP_TRIO + ("ragged_4099", "companion_5000")} == {2}
    assert GOLD["companion_5000"]["npx"] == 5000 and min((5000 + 3) & ~3, 4096) == 4096


def test_every_column_is_large_somewhere():
    """Thin rings and the dumbbells: the high-order moments are O(0.1), a wrong recombination coefficient is no noise."""
    best = np.max([GOLD[n]["exact"] for n in zc.CASES], axis=0)
    coeff = np.max([GOLD[n]["exact"] for n in zc.GROUPS["coeff"]], axis=0)
    print("largest value per column:", best)
    assert (best > 1e-3).all(), [zr.PAIRS[i] for i in np.flatnonzero(best <= 1e-3)]
    assert (coeff > 1e-3).all(), [zr.PAIRS[i] for i in np.flatnonzero(coeff <= 1e-3)]


def _ratios(featurize, names):
    """Worst |got - exact| / unit of each case through one CPU checker, each case alone."""
    out = {}
    s = _abi.default_settings(64)
    for name in names:
        got = featurize(zc.batch([name]), ZE, s)
        assert got.shape == (1, 30)
        out[name] = np.abs(got[0] - GOLD[name]["exact"]) / zr.UNITS
    return out


CHECKERS = ["oracle", "reference"]


@pytest.mark.parametrize("which", CHECKERS)
def test_the_reference_algorithm_stays_within_the_bound(which):
    if which == "reference" and not po.have_ref():
        pytest.skip("the reference classes are not built (oracle/_ref)")
    fn = po.oracle_featurize if which == "oracle" else po.ref_featurize
    for group, names in zc.GROUPS.items():
        ratio = _ratios(fn, names)
        worst = max(names, key=lambda n: ratio[n].max())
        print(f"{which} {group}: worst |got - exact| / unit = {ratio[worst].max():.2f} ({worst}, L = {zr.bound(GOLD[worst]['npx'])})")
        for name in names:
            L = zr.bound(GOLD[name]["npx"])
            assert (ratio[name] <= L).all(), (which, name, L, ratio[name].max(), zr.PAIRS[int(ratio[name].argmax())])
