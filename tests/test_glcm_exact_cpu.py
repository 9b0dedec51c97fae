"""The exact GLCM reference (tests/glcm_exact_ref.py) against the two CPU checkers, and the comparator against wrong matrices.

* The C oracle -- and the reference's own classes where they are built -- lie within K / 4 of the exact values on every case of
  tests/glcm_exact_cases.py (K = Ng^2 + 2 Ng + 64 units of 2^-53 x magnitude): the bound is not what lets them pass.  Degenerate,
  blank and soft_nan = -7.5 rows are equal by bits.
* Every case is sensitive: a lost, doubled or moved pair changes JAVE / SUMAVERAGE / CONTRAST / ACOR / DIS by at least 1000 times
  what the comparator tolerates.
* Five wrong matrices (a pair lost on a strip seam, a pair counted twice, a count moved to the transposed cell, to the neighbouring
  level, a seam row's pairs lost) are each reported by compare_glcm_exact; on the boxes with the most pairs the single-pair ones pass
  parity.compare_tables at 1e-5 -- the gap this suite closes, written down.

Worst |err| / (2^-53 magnitude) over all cases (profiles/glcm_exact_margin.txt, tools/glcm_exact_margin.py): see MARGIN below.
"""
import math

import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import glcm_exact_cases as gc
from tests import glcm_exact_ref as gx
from tests import parity

GLCM = _abi.FAM_GLCM
# measured on this suite's cases, quoted from profiles/glcm_exact_margin.txt: the largest ratio of any column against K of its case
MARGIN = ("oracle and reference classes: at most 0.124 K (ENERGY, 64 levels, 128 x 61 box, symmetric); HIP path, GLCM alone and INTENSITY + GLCM: "
          "at most 0.043 K (DIFVAR, radiomics binning, 4 occupied levels); the a-priori bound is 1.0 K, this module holds the CPU checkers to 0.25 K")


def _check_rows(table, c, names, soft_nan=0.0, tag="", scale=0.25):
    bad = []
    for r, e in enumerate(gc.exact(c, soft_nan)):
        bad += gx.compare_glcm_exact(table[r], e, e.Ng, names, len(e.request), tag="%sroi %d " % (tag, r), scale=scale)
    return bad


@pytest.mark.parametrize("c", gc.CASES, ids=lambda c: c.id)
def test_oracle_and_reference_classes_within_a_quarter_of_the_bound(c):
    b, s = gc.batch(c), c.settings()
    names = _lib.column_names(GLCM, s)
    bad = _check_rows(po.oracle_featurize(b, GLCM, s), c, names, tag="oracle ")
    if po.have_ref():
        bad += _check_rows(po.ref_featurize(b, GLCM, s, n_threads=4), c, names, tag="reference classes ")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("c", [c for c in gc.CASES if c.group == "S" or c.name in ("w129", "cloud300")], ids=lambda c: c.id)
def test_blank_and_soft_nan_rows_by_bits(c):
    """soft_nan = -7.5: blank angles (boxes one pixel wide or high, offsets beyond the box), CORRELATION without variance."""
    b, s = gc.batch(c), c.settings(-7.5)
    names = _lib.column_names(GLCM, s)
    ex = gc.exact(c, -7.5)
    if c.group == "S":
        assert any(a.blank for e in ex for a in e.angles), "the group has boxes whose angles have no pairs"
    bad = _check_rows(po.oracle_featurize(b, GLCM, s), c, names, soft_nan=-7.5, tag="oracle ")
    assert not bad, "\n".join(bad[:20])


def test_degenerate_row_is_zero_by_bits():
    """Binned minimum == binned maximum: the row is 0.0 whatever soft_nan is (constant ROI; 4094 and 4095 at 8 levels)."""
    yy, xx = np.mgrid[0:5, 0:7]
    rois = [dict(x=xx.ravel(), y=yy.ravel(), inten=np.full(35, 9, np.uint32)),
            dict(x=xx.ravel(), y=yy.ravel(), inten=(4094 + (xx.ravel() % 2)).astype(np.uint32))]
    b = _abi.batch_from_rois(rois)
    s = gc.settings(8, False, "usual", soft_nan=-7.5)
    names = _lib.column_names(GLCM, s)
    O = po.oracle_featurize(b, GLCM, s)
    for r in range(2):
        e = gx.exact_glcm(b, r, s)
        assert e.degenerate and all(v == 0.0 and not math.copysign(1, v) < 0 for v in e.value.values())
        assert not gx.compare_glcm_exact(O[r], e, e.Ng, names, 4)
        assert gx.compare_glcm_exact(np.full(len(names), -7.5), e, e.Ng, names, 4)


@pytest.mark.parametrize("c", gc.CASES, ids=lambda c: c.id)
def test_every_case_is_sensitive_to_one_pair(c):
    """The sensitivity condition, from the exact reference alone (glcm_exact_ref.sensitivity states the one exemption)."""
    for r, e in enumerate(gc.exact(c)):
        if e.degenerate:
            continue
        drop, move = gx.sensitivity(e)
        assert drop >= 1000 and move >= 1000, (c.id, r, int(gc.batch(c).bbox_w[r]), int(gc.batch(c).bbox_h[r]), drop, move)


# ---- mutations ------------------------------------------------------------------------------------------------------------

def _find(group, name=None, **kw):
    return next(c for c in gc.CASES if c.group == group and (name is None or c.name == name) and all(getattr(c, k) == v for k, v in kw.items()))


def _roi_of(c, w):
    b = gc.batch(c)
    return next(r for r in range(b.n_roi) if int(b.bbox_w[r]) == w)


# (case, box width): three boxes of the large-ROI path and one of the smallest class
MUTATED = [(("L", dict(gd=8, request="sym")), 129), (("L", dict(gd=8, request="off2")), 20000), (("L", dict(gd=-16, request="usual")), 4100),
           (("S", dict(gd=8, request="usual")), 16)]


def _mutants(c, r, b=None, e=None):
    """{name: matrices} -- the exact matrices of row r with one error each, all in the 90-degree angle (the pairs that cross a strip
    seam): the seam lies between rows rps - 1 and rps of the box (small boxes: between rows 3 and 4)."""
    s = c.settings()
    b = gc.batch(c) if b is None else b
    e = gc.exact(c)[r] if e is None else e
    k90 = e.request.index(90)
    plane = gx.dense_plane(b, r)
    idx, I, grey_info = gx.levels_of(plane, int(b.min_inten[r]), int(b.max_inten[r]), s)
    sym = bool(s.glcm_symmetric) or grey_info <= 0
    off = int(s.glcm_offset)
    h, w = plane.shape
    rps = max(1, gc.STRIP_CELLS // w) if c.group == "L" else 4
    top = min(rps, h - off) - 1                                        # the centre row of the seam pairs
    M = e.angles[k90].M
    # a seam pair between two DIFFERENT levels, both counted, nearest the middle of the level range
    cand = [(abs(2 * idx[top, x] - len(I)) + abs(2 * idx[top + off, x] - len(I)), x) for x in range(w)
            if idx[top, x] >= 0 and idx[top + off, x] >= 0 and idx[top, x] != idx[top + off, x]]
    x = min(cand)[1]
    lc, ln = int(idx[top, x]), int(idx[top + off, x])

    def with_(dM):
        return [a.M + dM if k == k90 else a.M for k, a in enumerate(e.angles)]

    def cell(r_, c_, v):
        d = np.zeros_like(M)
        d[r_, c_] += v
        if sym:
            d[c_, r_] += v
        return d
    seam_row = gx.cooc_matrix(idx[top:top + off + 1][[0, off]], len(I), 0, 1, sym)   # the pairs centred on row `top`
    ln2 = ln + 1 if ln + 1 < len(I) and ln + 1 != lc else ln - 1
    out = {"pair lost on the seam": with_(cell(lc, ln, -1)),
           "pair counted twice": with_(cell(lc, ln, 1)),
           "count moved to the neighbouring level": with_(cell(lc, ln, -1) + cell(lc, ln2, 1)),
           "seam row lost": with_(-seam_row)}
    if not sym:
        out["count moved to the transposed cell"] = with_(cell(lc, ln, -1) + cell(ln, lc, 1))
    else:                                                              # (a symmetric matrix has no transposed cell to err to: one direction of the pair lost)
        d = np.zeros_like(M)
        d[lc, ln] -= 1
        out["count moved to the transposed cell"] = with_(d)
    assert all((m >= 0).all() for ms in out.values() for m in ms)
    return e, I, out


@pytest.mark.parametrize("which,width", MUTATED, ids=["%s-gd%d-%s-w%d" % (g, kw["gd"], kw["request"], w) for (g, kw), w in MUTATED])
def test_wrong_matrices_are_reported(which, width):
    c = _find(which[0], **which[1])
    r = _roi_of(c, width)
    s = c.settings()
    names = _lib.column_names(GLCM, s)
    e, I, mutants = _mutants(c, r)
    right = gx.row_from_matrices([a.M for a in e.angles], I, e.request, names)
    assert not gx.compare_glcm_exact(right, e, e.Ng, names, len(e.request)), "the unmutated matrices reproduce the reference"
    for what, mats in mutants.items():
        row = gx.row_from_matrices(mats, I, e.request, names)
        bad = gx.compare_glcm_exact(row, e, e.Ng, names, len(e.request))
        assert any("_90:" in m for m in bad) and any("_AVE:" in m for m in bad), (c.id, what, bad[:3])


def test_errors_pass_the_relative_comparison_at_the_pair_count_of_a_large_roi():
    """The gap, written down.  The matrices of a 129 x 127 box (a skewed ramp under noise) scaled by 50 -- 800 000 pairs an angle, what a 400 k-pixel ROI has --
    with the same five errors: a pair lost, doubled or moved changes every column by about 1e-6 relative, and parity.compare_tables
    (1e-5) passes the table computed from the wrong matrix; compare_glcm_exact reports every one of them.  (At the 16 000 pairs of the
    129-wide box itself 1e-5 still sees a single pair in one column or another: the boxes of this suite are small so that they are
    quick, the gap is at the benchmark's sizes.  The lost seam row -- 129 pairs -- is asserted on the exact side only.)"""
    c = _find("L", gd=8, request="usual")
    d = gc.roi(129, 127, "noise", np.random.default_rng(5))
    # smooth and skewed: neighbours correlate and the third moment is far from 0, so no column is a sum that cancels to nearly nothing
    # (on plain noise CORRELATION and CLUSHADE are, and 1e-5 of a value near 0 does see one pair in 800 000)
    ramp = 4095.0 * (d["x"] + d["y"]) / 254.0
    d["inten"] = (1 + (0.7 * ramp + 0.3 * d["inten"]) ** 2 // 4095).astype(np.uint32)
    b = _abi.batch_from_rois([d])
    names = _lib.column_names(GLCM, c.settings())
    e, I, mutants = _mutants(c, 0, b, gx.exact_glcm(b, 0, c.settings()))
    big = [50 * a.M for a in e.angles]
    k90 = e.request.index(90)
    right = gx.row_from_matrices(big, I, e.request, names)
    ex = gx.GlcmExact()
    ex.degenerate, ex.Ng, ex.request, ex.bits = False, len(I), e.request, set()
    ang = [gx.exact_angle(M, I, 0.0) for M in big]
    ex.value = {n: v for n, v in zip(names, right) if not np.isnan(v)}
    ex.magnitude = {}
    for n in ex.value:
        col, suf = n[5:].rsplit("_", 1)
        ex.magnitude[n] = sum(a.magnitude[col] for a in ang) / len(ang) if suf == "AVE" else ang[e.request.index(int(suf))].magnitude[col]
    for what, mats in mutants.items():
        wrong = [50 * a.M + (m - a.M) for a, m in zip(e.angles, mats)]            # the same error on the scaled matrix
        row = gx.row_from_matrices(wrong, I, e.request, names)
        assert any("_90:" in m for m in gx.compare_glcm_exact(row, ex, ex.Ng, names, len(e.request))), what
        blind = not parity.compare_tables(row[None], right[None], names)
        assert blind or what == "seam row lost", (what, parity.compare_tables(row[None], right[None], names)[:3])
