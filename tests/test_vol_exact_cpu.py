"""The exact 3-D GLCM reference (tests/vol_exact_ref.py) without a GPU.

* Reference held: the values recorded from the reference's own 3-D classes (tests/golden/vol, all 15 cases) and the NumPy restatement
  (vol_ref.table) lie within SCALE = 0.25 of the bound K(Ng) 2^-53 magnitude in every rational column; blank directions, NaN
  CORRELATIONs and rows without voxels are equal by bits.  Measured worst over the 15 recorded cases: 0.041 K (ASM, blob40 under
  cap_matlab, Ng 128) -- profiles/vol_glcm_exact_margin.txt, tools/vol_glcm_exact_margin.py -- so 0.25 leaves a factor of six.
* Sensitivity: on every GLCM case of tests/vol_edge_cases.py a lost, doubled or moved pair is at least 1000 times the tolerance.
* Mutants: a pair dropped, doubled, moved to a neighbouring cell, two directions' matrices swapped, and the asymmetric matrix where the
  symmetric one is due are each reported by compare_vol_exact on a w = 33 box, a needle and the 65-level ROI; at the pair count of a
  large volume (the needle's matrices scaled by 50) the one-pair mutants pass vol_cases.compare at 1e-5 -- the gap this suite closes.
* The edge cases hold what they are named for: widths on both sides of every switch of the lane-sharing rule, row counts around the
  row loop's stride, border pairs of the negative shifts, cells % 4, level sets, blank directions of the offsets, pass counts of
  the sort, run layouts of the mode search and which wave owns a run's head.
"""
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

from nyxus_amd import _abi
from tests import glcm_exact_ref as gx
from tests import vol_cases, vol_edge_cases as ve, vol_exact_ref as vx, vol_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "vol", "vol_reference.npz")
N_INT = vol_cases.N_INT
NAMES = vx.glcm_names()
SCALE = 0.25                       # what the reference's classes and the restatement are held to; the a-priori bound is 1.0


def test_column_layout_is_feature3d_order():
    assert NAMES == vol_cases.column_names()[N_INT:]
    assert NAMES[:14] == ["3GLCM_ACOR_%d" % d for d in range(13)] + ["3GLCM_ASM_0"] and NAMES[390] == "3GLCM_ASM_AVE" and len(NAMES) == 419
    e = vx.exact_row(vol_cases.batch("boxes"), 4, vol_cases.settings("matlab"))
    assert set(e.value) == {n for n in NAMES if n.split("_")[1] not in gx.LOG_COLUMNS} and len(e.value) == 24 * 13 + 23


@functools.lru_cache(maxsize=None)
def _held(bname, mode):
    """(mismatches at SCALE, worst ratio / K of the reference's classes, exact rows) of a recorded case."""
    b, s = vol_cases.batch(bname), vol_cases.settings(mode)
    rows = vx.exact_rows(b, s)
    recorded = np.load(GOLD)[vol_cases.case_name(bname, mode)][:, N_INT:]
    worst = 0.0
    bad = []
    for r, e in enumerate(rows):
        ratios = {}
        bad += vx.compare_vol_exact(recorded[r], e, e.Ng, NAMES, ratios=ratios, tag="reference classes roi %d " % r, scale=SCALE)
        worst = max([worst] + [v / vx.K(e.Ng) for v in ratios.values()])
    bad += vx.compare_table(vol_ref.table(b, s, _abi.VFAM_GLCM), rows, NAMES, tag="vol_ref ", scale=SCALE)
    return bad, worst, rows


@pytest.mark.parametrize("bname,mode", vol_cases.CASES)
def test_reference_classes_and_restatement_within_a_quarter_of_the_bound(bname, mode):
    bad, worst, rows = _held(bname, mode)
    print(f"{bname}/{mode}: worst |err| / (K 2^-53 magnitude) of the reference's classes {worst:.4f}")
    assert not bad, "\n".join(bad[:20])
    # the flat ROIs under radiomics binning are all-blank rows
    ex = vol_cases.rule_excluded(vol_cases.batch(bname), vol_cases.settings(mode))[:, N_INT:].all(axis=1)
    assert all(all(a.blank for a in rows[r].angles) for r in np.flatnonzero(ex))


def test_the_margin_leaves_a_factor_of_two():
    """SCALE is asserted where the measured worst of the reference's classes over the 15 recorded cases stays below half of it."""
    worst = {c: _held(*c)[1] for c in vol_cases.CASES}
    assert len(worst) == 15 and 0 < max(worst.values()) < SCALE / 2, worst


def test_three_d_specifics_by_bits():
    b = vol_cases.with_empty(vol_cases.batch("boxes"), at=5)
    rows = vx.exact_rows(b, vol_cases.settings("softnan"))                   # radiomics binning, soft_nan = -7.5
    sn = np.float64(-7.5)
    assert rows[5].empty and all(gx._same_bits(v, sn) for v in rows[5].value.values()) and rows[5].bits == set(rows[5].value)
    e = rows[0]                                                              # 1x1x1: no pair in any direction, no degenerate-row guard: soft_nan, not 0
    assert all(a.blank for a in e.angles) and all(v == -7.5 for n, v in e.value.items() if not n.endswith("_AVE"))
    assert all(abs(v + 7.5) <= e.tol[n] and e.tol[n] <= 14 * 7.5 * vx.EPS for n, v in e.value.items() if n.endswith("_AVE"))
    flat = rows[10]                                                          # the flat 3x3x2 patch (row 9 before the insertion) under radiomics binning
    assert all(a.blank for a in flat.angles) and flat.Ng == 0
    # 2x1x1 under matlab binning: one pair in (1, 0, 0), one cell, so each marginal has one level: 0 / 0
    e = vx.exact_row(b, 1, ve.settings((("glcm_grey_depth", 16), ("soft_nan", -7.5))))
    assert [a.blank for a in e.angles] == [d != 4 for d in range(13)] and e.Ng == 16
    assert np.isnan(e.value["3GLCM_CORRELATION_4"]) and "3GLCM_CORRELATION_4" in e.bits
    assert np.isnan(e.value["3GLCM_CORRELATION_AVE"]) and "3GLCM_CORRELATION_AVE" in e.bits
    # _AVE: the exact mean, a blank direction contributing soft_nan
    assert e.value["3GLCM_JAVE_AVE"] == float((12 * Fraction(-15, 2) + e.angles[4].frac["JAVE"]) / 13)
    got = vx.table_row(e)
    assert not vx.compare_vol_exact(got, e, e.Ng, NAMES)
    got[NAMES.index("3GLCM_CORRELATION_4")] = -7.5                           # the guard of the 2-D class
    assert len(vx.compare_vol_exact(got, e, e.Ng, NAMES)) == 1
    with pytest.raises(AssertionError):
        vx.compare_vol_exact(got, e, e.Ng, NAMES, scale=1.5)


@pytest.mark.parametrize("c", ve.GLCM_CASES, ids=lambda c: c.id)
def test_every_edge_case_is_held_and_sensitive_to_one_pair(c):
    """vol_ref's restatement lies within SCALE on the case, and the sensitivity condition holds (rows that compare by bits -- no pairs in any
    direction -- are excepted: glcm_exact_ref.sensitivity answers inf for them)."""
    b = ve.batch(c.bname)
    rows = ve.exact(c)
    bad = vx.compare_table(ve.reference(c), rows, NAMES, tag="vol_ref ", scale=SCALE)
    assert not bad, "\n".join(bad[:20])
    for r, e in enumerate(rows):
        drop, move = vx.sensitivity(e)
        assert drop >= 1000 and move >= 1000, (c.id, r, int(b.bbox_w[r]), int(b.bbox_h[r]), int(b.bbox_d[r]), drop, move)


# ---- mutants ----------------------------------------------------------------------------------------------------------------

def _find(group, name):
    return next(c for c in ve.GLCM_CASES if c.group == group and c.name == name)


# (case, row, direction): a w = 33 box, the needle along x, the 65-level ROI -- every one of them counted symmetrically
MUTATED = [(_find("widths", "radiomics16"), 2 * ve.WIDTHS.index(33), 0), (_find("needles", "matlab64_sym"), 0, 4), (_find("levels", "ibsi_64_65_128"), 1, 7)]


def _one_sided(b, r, s):
    """The 13 matrices of row r counted in one direction only (what the symmetric count is the sum of, with its transpose)."""
    D, g = vx.level_box(b, r, s)
    I = vx.matrices(b, r, s)[1]
    rank = np.zeros(max(int(D.max()), int(I.max())) + 1, np.int64)
    rank[I] = np.arange(1, len(I) + 1)                                       # level -> 1 + matrix index, 0 stays 0
    return [vol_ref.cooc(rank[D], sh, int(s.glcm_offset), len(I), False)[0] for sh in vol_cases.SHIFTS]


def _mutants(c, r, d):
    b, s = ve.batch(c.bname), ve.settings(c.mode)
    e = ve.exact(c)[r]
    mats, I = vx.matrices(b, r, s)
    M = mats[d]
    # an off-diagonal occupied cell nearest the middle of the level range
    cells = [(abs(2 * i - len(I)) + abs(2 * j - len(I)), i, j) for i, j in zip(*np.nonzero(M)) if i != j]
    _, i, j = min(cells)
    j2 = j + 1 if j + 1 < len(I) and j + 1 != i else j - 1

    def cell(i_, j_, v):
        dM = np.zeros_like(M)
        dM[i_, j_] += v
        dM[j_, i_] += v
        return dM

    def with_(Md):
        return [Md if k == d else m for k, m in enumerate(mats)]
    one = _one_sided(b, r, s)
    assert all((o + o.T == m).all() for o, m in zip(one, mats)), "the case counts symmetrically"
    other = next(k for k in range(13) if k != d and (mats[k] != M).any())          # (the needle's other directions are blank)
    swapped = list(mats)
    swapped[d], swapped[other] = mats[other], mats[d]
    out = {"pair dropped": with_(M + cell(i, j, -1)), "pair doubled": with_(M + cell(i, j, 1)),
           "pair moved to a neighbouring cell": with_(M + cell(i, j, -1) + cell(i, j2, 1)),
           "directions %d and %d swapped" % (d, other): swapped, "asymmetric matrix": with_(one[d])}
    assert all((m >= 0).all() for ms in out.values() for m in ms)
    return e, I, mats, out


def _closed_row(mats, I, soft_nan=0.0):
    """The GLCM block a kernel that counted `mats` would report: vol_ref's closing formulas in doubles, all 30 codes and the _AVE."""
    vals = np.zeros((13, 30))
    for k, M in enumerate(mats):
        f = vol_ref.close(M, I, soft_nan)
        vals[k] = [f[c] for c in vol_ref.ANG_3D]
    return np.concatenate([vals.T.ravel(), [vol_ref.reduce13(vals[:, vol_ref.ANG_3D.index(c)]) for c in vol_ref.AVE_3D]])


@pytest.mark.parametrize("c,r,d", MUTATED, ids=["w33", "needle", "65levels"])
def test_wrong_matrices_are_reported(c, r, d):
    e, I, mats, mutants = _mutants(c, r, d)
    b = ve.batch(c.bname)
    assert (int(b.bbox_w[r]) == 33 or c.group != "widths") and e.Ng == len(I) and (e.Ng == 65 or c.group != "levels")
    for make in (vx.row_from_matrices, _closed_row):                         # from the exact values, and from the closing formulas in doubles
        right = make(mats, I)
        assert not vx.compare_vol_exact(right, e, e.Ng, NAMES), "the unmutated matrices reproduce the reference"
        for what, ms in mutants.items():
            bad = vx.compare_vol_exact(make(ms, I), e, e.Ng, NAMES)
            assert any("_%d:" % d in m for m in bad), (c.id, what, bad[:3])
            # (the mean over the directions does not change when two of them change places)
            assert "swapped" in what or any("_AVE:" in m for m in bad), (c.id, what, bad[:3])


def test_one_pair_passes_the_relative_comparison_at_the_pair_count_of_a_large_volume():
    """The gap, written down.  The needle's matrices scaled by 50 -- 6.5 million counted pairs in its direction, what a box of 190^3 cells
    has -- with the same one-pair errors: every column moves by less than 1e-5 relative, and vol_cases.compare passes the row computed from
    the wrong matrix; compare_vol_exact reports each.  (At the 131 066 pairs of the needle itself 1e-5 still sees a single pair in the
    columns that cancel, CLUSHADE first: the cases of this suite are small so that they are quick, the gap is at the sizes of real volumes.)"""
    c, r, d = MUTATED[1]
    e, I, mats, mutants = _mutants(c, r, d)
    assert e.angles[d].N == 2 * 65533
    big = [50 * m for m in mats]
    eb = vx.from_matrices(big, I, 0.0)
    right = _closed_row(big, I)
    assert not vx.compare_vol_exact(right, eb, eb.Ng, NAMES)
    for what in ("pair dropped", "pair doubled", "pair moved to a neighbouring cell"):
        row = _closed_row([bm + (w - m) for bm, w, m in zip(big, mutants[what], mats)], I)      # the same error on the scaled matrix
        bad = vx.compare_vol_exact(row, eb, eb.Ng, NAMES)
        assert any("_%d:" % d in m for m in bad) and any("_AVE:" in m for m in bad), what
        blind, _, rg = vol_cases.compare(row[None], right[None], NAMES)
        assert not blind and 0 < rg < 1e-5, (what, rg, blind[:3])


# ---- the cases hold what they are named for ---------------------------------------------------------------------------------

def _boxes(b):
    return list(zip(b.bbox_w.tolist(), b.bbox_h.tolist(), b.bbox_d.tolist()))


def test_widths_and_rows_lie_on_both_sides_of_every_switch():
    b = ve.batch("widths")
    assert _boxes(b) == [(w, 3, 3) for w in ve.WIDTHS for _ in range(2)]
    full = b.counts() == b.cells()
    assert full[0::2].all() and not full[1::2].any() and (b.counts()[1::2] > 0.5 * b.cells()[1::2]).all()
    assert [ve.lane_width(w) for w in ve.WIDTHS] == [8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 64, 64, 64, 64]
    assert {(w - 1) // 64 for w in ve.WIDTHS} == {0, 1, 2}                                # one, two and three trips of the x loop
    rb = ve.row_boxes()
    assert _boxes(ve.batch("rows")) == rb
    for w, rpw in ((8, 8), (64, 1)):
        assert 64 // ve.lane_width(w) == rpw
        prods = sorted({h * d for ww, h, d in rb if ww == w})
        assert prods == [4 * rpw - 1, 4 * rpw, 4 * rpw + 1, 8 * rpw + 1]
        for p in prods:
            shapes = {(h, d) for ww, h, d in rb if ww == w and h * d == p}
            assert (p, 1) in shapes and (1, p) in shapes
        assert any(h > 1 and d > 1 for ww, h, d in rb if ww == w)


def test_negative_shifts_have_pairs_at_both_borders():
    """Every direction with a negative dy or dz: emptying either border plane of that axis takes pairs out of its matrix."""
    for c in ve.of_group("negshift"):
        b, s = ve.batch(c.bname), ve.settings(c.mode)
        for r in range(b.n_roi):
            D, g = vx.level_box(b, r, s)
            mats, I = vx.matrices(b, r, s)
            for k, (dx, dy, dz) in enumerate(vol_cases.SHIFTS):
                for axis, comp in ((1, dy), (0, dz)):
                    if comp >= 0:
                        continue
                    for plane in (0, D.shape[axis] - 1):
                        E = D.copy()
                        E[(slice(None),) * axis + (plane,)] = 0
                        P = vol_ref.cooc(E, (dx, dy, dz), int(s.glcm_offset), g, bool(s.glcm_symmetric))[0]
                        assert P.sum() < mats[k].sum(), (c.id, r, k, axis, plane)


def test_tail_words_and_seam_cells():
    b = ve.batch("tail")
    assert _boxes(b) == list(ve.TAIL_BOXES) and sorted(set((b.cells() % 4).tolist())) == [0, 1, 2, 3]
    assert {int(c % 4) for c in b.cells() if c > 1024} == {0, 1, 2, 3}                    # ... and again beyond one trip of 256 words
    off = b.px_offset.astype(np.int64)
    for r, (w, h, d) in enumerate(_boxes(b)):
        sl = slice(off[r], off[r + 1])
        assert ((b.x[sl] == w - 1) & (b.y[sl] == h - 1) & (b.z[sl] == d - 1)).any(), "the last cell is occupied"
    assert int(b.max_inten.max()) <= vol_cases.LEVEL_CAP                                  # serves in IBSI mode
    assert [ve.settings(c.mode).glcm_symmetric for c in ve.of_group("tail")] == [0, 1, 0] and ve.settings(ve.of_group("tail")[2].mode).ibsi == 1
    assert vx.level_box(b, 0, ve.settings(ve.of_group("tail")[0].mode))[0].min() == 1     # matlab binning: the background is level 1
    assert sorted(ve.batch("seam").cells()) == [32767, 32768, 32769] and list(ve.batch("blob40").cells()) == [64000]
    assert _boxes(ve.batch("seam33")) == [(33, 32, 31), (64, 32, 16)] and list(ve.batch("seam33").cells()) == [32736, 32768]
    assert 32768 - 32736 < 33                                                              # no multiple of 33 lies nearer below the seam


def _levels(c):
    b, s = ve.batch(c.bname), ve.settings(c.mode)
    return [sorted(set(np.unique(vx.level_box(b, r, s)[0]).tolist()) - {0}) for r in range(b.n_roi)]


def test_level_sets_straddle_the_presence_map():
    by = {c.name: c for c in ve.of_group("levels")}
    assert _levels(by["radiomics_63_to_66"]) == [[63, 64, 65, 66]]
    assert _levels(by["radiomics_128"]) == [[1, 64, 65, 128], list(range(1, 129))]
    L = _levels(by["ibsi_64_65_128"])
    assert L[:3] == [list(range(1, 65)), list(range(1, 66)), list(range(1, 129))] and L[3] == [65]
    assert [e.Ng for e in ve.exact(by["ibsi_64_65_128"])] == [64, 65, 128, 65]
    assert [e.Ng for e in ve.exact(by["radiomics_63_to_66"]) + ve.exact(by["radiomics_128"])] == [4, 4, 128]
    b = ve.batch("levels_ibsi")
    assert (b.inten[b.px_offset[3]:] == 0).any()                                           # the 65-only ROI has cells that are not counted
    assert ve.settings(by["matlab128"].mode).glcm_grey_depth == 128 == vol_cases.LEVEL_CAP and ve.exact(by["matlab128"])[0].Ng == 128
    m = _levels(by["matlab128"])[0]
    assert min(m) == 1 and max(m) == 128 and len(m) > 100


def test_offsets_blank_what_they_should():
    live = {c.name: [k for k, a in enumerate(ve.exact(c)[0].angles) if not a.blank] for c in ve.of_group("offsets")}
    assert _boxes(ve.batch("off_9x4x3")) == [(9, 4, 3)]
    assert live["9x4x3_offset1"] == list(range(13)) and live["9x4x3_offset2"] == list(range(13))
    assert live["9x4x3_offset8"] == [4] and live["9x4x3_offset9"] == [] and live["9x4x3_offset10"] == []   # w - 1: (1, 0, 0) alone; w, w + 1: none
    assert _boxes(ve.batch("off_depth2")) == [(7, 6, 2)] and live["depth2_offset3"] == [1, 4, 7, 10]      # every dz != 0 direction blank
    assert _boxes(ve.batch("off_310")) == [(310, 2, 2)] and live["310x2x2_offset300"] == [4]
    assert ve.settings(_find("offsets", "310x2x2_offset300").mode).glcm_offset == 300 > 256


def test_needles():
    b = ve.batch("needles")
    assert _boxes(b) == [(65534, 1, 1), (1, 65534, 1), (1, 1, 65534)] and (b.counts() == 65534).all() and 32 <= int(b.inten.max()) < 64
    assert int(b.x.max()) == int(b.y.max()) == int(b.z.max()) == 65533


def test_sort_rois_cross_sizes_and_pass_counts():
    b = ve.batch("sort")
    vals = ve.sort_values()
    assert b.n_roi == 180 and [(n, bits) for n, bits, _ in vals] == [(n, bits) for n in ve.SORT_N for bits in ve.SORT_BITS]
    off = b.px_offset.astype(np.int64)
    passes = set()
    for k, (n, bits, v) in enumerate(vals):
        a, d = b.inten[off[2 * k]:off[2 * k + 1]], b.inten[off[2 * k + 1]:off[2 * k + 2]]
        assert len(a) == n and (a == v).all() and (d == v[::-1]).all() and (np.diff(a.astype(np.int64)) >= 0).all()
        rg = int(b.max_inten[2 * k]) - int(b.min_inten[2 * k])
        assert int(a.min()) == int(b.min_inten[2 * k]) and int(a.max()) == int(b.max_inten[2 * k])          # min and max are attained
        assert rg.bit_length() == (bits if n > 1 else 0)                                                     # 32 - clz(range)
        passes.add(((rg.bit_length() + 3) // 4, -(-n // 256)))
    # every pass count 0..8, odd ones (the second buffer ends up as the table) and even ones, at one, two, three and five keys a thread
    assert {p for p, _ in passes} == {0, 1, 2, 3, 4, 8} and {cs for _, cs in passes} == {1, 2, 3, 5}
    assert {(p % 2, cs) for p, cs in passes if p} >= {(1, 1), (0, 1), (1, 2), (0, 2), (1, 3), (0, 3)}
    big = ve.batch("sort4097")
    assert big.counts()[0] == 4097 and int(big.max_inten[0]) - int(big.min_inten[0]) == 2 ** 32 - 1
    for r, (n, bits) in zip(ve.BINS_ROIS, ((256, 8), (512, 16), (1025, 32))):
        assert b.counts()[r] == n and (int(b.max_inten[r]) - int(b.min_inten[r])).bit_length() == bits


def test_mode_layouts():
    b = ve.batch("mode")
    off = b.px_offset.astype(np.int64)
    heads = {}
    for r, (name, (lengths, mode_run)) in enumerate(ve.MODE_LAYOUTS.items()):
        v = np.sort(b.inten[off[r]:off[r + 1]])
        u, first, cnt = np.unique(v, return_index=True, return_counts=True)
        assert cnt.tolist() == list(lengths), name
        best = int(np.flatnonzero(cnt == cnt.max())[0])                                   # the smallest value among the longest runs
        assert best == mode_run, name
        heads[name] = [int(i) for i in first[cnt == cnt.max()]]
    wave = lambda i: (i % 256) // 64                                                       # the wave whose stride owns index i
    assert [max(l) for l, _ in list(ve.MODE_LAYOUTS.values())[:11]] == [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257]
    n_end = sum(ve.MODE_LAYOUTS["ends_at_n"][0])
    assert heads["ends_at_n"] == [n_end - 7] and heads["starts_at_0"] == [0]
    assert [wave(i) for i in heads["tie2"]] == [3, 0] and heads["tie2"][1] >= 256          # the smaller value's head in a later wave
    assert [wave(i) for i in heads["tie2_same_trip"]] == [1, 3] and heads["tie2_same_trip"][1] < 256
    assert [wave(i) for i in heads["tie3"]] == [2, 0, 1]
    assert max(ve.MODE_LAYOUTS["long700"][0]) == 700 > 256
    assert ve.MODE_LAYOUTS["pow2_1023"][0][5:8] == [1023, 1024, 1025]


def test_chunk_batch_crosses_the_grid_bound():
    b = ve.batch("chunk")
    assert b.n_roi == ve.CHUNK_ROIS == 65550 and b.n_roi > 65535
    p = vol_cases.batch("boxes")
    for r in (0, 11, 12, 65534, 65535, 65536, 65549):
        one, pat = b.select([r]), p.select([r % 12])
        assert all((getattr(one, k) == getattr(pat, k)).all() for k in ("x", "y", "z", "inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten"))
