"""Exact reference for the 3-D GLCM columns, and the comparator that holds a volume table to it (CPU only; loads no HIP library).

The level box is built the way vol_ref.glcm_rows builds it (background level from the binning mode, voxels from the cloud), the
integer matrix of each of the 13 directions comes from vol_ref.cooc, and the 24 rational columns of a direction come from
glcm_exact_ref.exact_angle -- the 2-D module's routine, reused as it stands, handed NaN as its `soft_nan` argument the way the
kernel hands it to the shared closing routine for the two quotients the 3-D class leaves unguarded.  What is 3-D about the row:

  * a direction without pairs is 30 x soft_nan by bits; CORRELATION with a zero denominator is NaN by bits; there is no
    degenerate-row guard; a flat ROI under radiomics binning has level 0 everywhere, so every direction is blank
    (vol_cases.rule_excluded); an ROI without voxels is a row of soft_nan;
  * Feature3D order: ACOR before ASM, column code * 13 + direction, then the 29 _AVE columns;
  * _AVE is the exact mean of the 13 directional values as rationals, a blank direction contributing soft_nan as an exact value, NaN by
    bits if any direction is NaN.  Its tolerance is (sum of the 13 directional tolerances + 13 x 2^-53 x sum |v_k|) / 13: twelve
    additions in any order and one division, each rounding at most 2^-53 of the running magnitude (<= sum |v_k|).  Derived, not tuned.

compare_vol_exact grants |got - exact| <= scale * K(Ng) * 2^-53 * magnitude with scale <= 1 asserted (glcm_exact_ref's K and magnitudes;
compare_glcm_exact's contract, `ratios` included).  Ng is the matrix order of the ROI: g under matlab binning, the largest level under
IBSI, the distinct-level count under radiomics binning.  The six log columns stay on vol_cases.compare against vol_ref.
"""
from __future__ import annotations

import math

import mpmath
import numpy as np

from tests import glcm_exact_ref as gx
from tests import vol_ref
from tests.vol_cases import N_DIR, SHIFTS

EPS = gx.EPS
K = gx.K
EXACT = gx.EXACT                                         # the 24 rational columns (CORRELATION with its two square roots among them)
LOG_COLUMNS = gx.LOG_COLUMNS
NAN = float("nan")


def level_box(b, r, s):
    """(D[z, y, x] of levels, grey_info) of row r: vol_ref.glcm_rows's box."""
    g = 0 if s.ibsi else int(s.glcm_grey_depth)
    off = b.px_offset.astype(np.int64)
    sl = slice(off[r], off[r + 1])
    w, h, d = int(b.bbox_w[r]), int(b.bbox_h[r]), int(b.bbox_d[r])
    mn, mx = int(b.min_inten[r]), int(b.max_inten[r])
    bg = vol_ref.bin_levels(np.zeros(1, np.uint32), mn, mx, g)[0]
    D = np.full((d, h, w), bg, np.int64)
    D[b.z[sl], b.y[sl], b.x[sl]] = vol_ref.bin_levels(b.inten[sl], mn, mx, g)
    return D, g


def matrices(b, r, s, D=None):
    """([13 int64 matrices], level values I) of row r under s (D: a level box to use instead of the row's own)."""
    D0, g = level_box(b, r, s)
    D = D0 if D is None else D
    out, I = [], None
    for sh in SHIFTS:
        P, I = vol_ref.cooc(D, sh, int(s.glcm_offset), g, bool(s.glcm_symmetric))
        out.append(P)
    return out, np.asarray(I, np.int64)


class VolExact:
    """One ROI under one Settings.  Ng: matrix order.  angles: the 13 directions (glcm_exact_ref.Angle; .blank: no pairs).  value / tol /
    magnitude: per column NAME of the table ('3GLCM_ASM_4', '3GLCM_ASM_AVE') the expected double, the tolerance at scale 1 and the
    magnitude; ave_round: the part of an _AVE tolerance that does not scale (13 x 2^-53 x sum |v_k| / 13); bits: the names that compare by
    bits; empty: no voxels.  degenerate / request are there for glcm_exact_ref.sensitivity, which reads them."""


def _blank_angle(soft_nan):
    return gx.exact_angle(np.zeros((0, 0), np.int64), np.zeros(0, np.int64), soft_nan)


def from_matrices(mats, I, soft_nan, empty=False) -> VolExact:
    """The exact row of 13 direction matrices over the level values I."""
    e = VolExact()
    e.empty, e.degenerate, e.request = empty, False, list(range(N_DIR))
    e.Ng = len(I)
    e.value, e.tol, e.magnitude, e.ave_round, e.bits = {}, {}, {}, {}, set()
    soft_nan = float(soft_nan)
    e.angles = []
    for M in mats:
        M = np.asarray(M, np.int64)
        # the blank direction is answered here (30 x soft_nan); exact_angle's own use of its argument is then the two unguarded quotients
        e.angles.append(_blank_angle(soft_nan) if empty or M.sum() == 0 else gx.exact_angle(M, np.asarray(I, np.int64), NAN))
    k = K(e.Ng)
    for c in EXACT:
        for d, a in enumerate(e.angles):
            n = "3GLCM_%s_%d" % (c, d)
            e.value[n], e.magnitude[n] = a.value[c], a.magnitude[c]
            e.tol[n] = k * EPS * a.magnitude[c]
            if c in a.bits:
                e.bits.add(n)
        if c in gx.NO_AVE:
            continue
        n = "3GLCM_%s_AVE" % c
        vals = [a.value[c] for a in e.angles]
        if empty:
            e.value[n], e.magnitude[n], e.tol[n], e.ave_round[n] = soft_nan, 0.0, 0.0, 0.0
            e.bits.add(n)
        elif any(math.isnan(v) for v in vals):
            e.value[n], e.magnitude[n], e.tol[n], e.ave_round[n] = NAN, 0.0, 0.0, 0.0
            e.bits.add(n)
        else:
            if c == "CORRELATION":
                with mpmath.workprec(200):
                    v = float(sum(a.frac[c] for a in e.angles) / N_DIR)
            else:
                v = sum(a.frac[c] for a in e.angles) / N_DIR
                v = v.numerator / v.denominator
            e.value[n] = v
            e.magnitude[n] = sum(a.magnitude[c] for a in e.angles) / N_DIR
            e.ave_round[n] = N_DIR * EPS * sum(abs(x) for x in vals) / N_DIR
            e.tol[n] = sum(e.tol["3GLCM_%s_%d" % (c, d)] for d in range(N_DIR)) / N_DIR + e.ave_round[n]
    return e


def exact_row(b, r, s) -> VolExact:
    """The exact GLCM columns of row r of HostBatch3D b under Settings s."""
    if int(b.px_offset[r + 1]) == int(b.px_offset[r]):
        return from_matrices([np.zeros((0, 0), np.int64)] * N_DIR, np.zeros(0, np.int64), s.soft_nan, empty=True)
    mats, I = matrices(b, r, s)
    return from_matrices(mats, I, s.soft_nan)


def exact_rows(b, s):
    return [exact_row(b, r, s) for r in range(b.n_roi)]


def glcm_names():
    """The GLCM block's column names in Feature3D order (what nyxhip_vol_column_name answers under VFAM_GLCM)."""
    return ["3GLCM_%s_%d" % (c, d) for c in vol_ref.ANG_3D for d in range(N_DIR)] + ["3GLCM_%s_AVE" % c for c in vol_ref.AVE_3D]


def table_row(e: VolExact, names=None):
    """The exact columns of e laid out under `names` (NaN where the exact reference has no value: the log columns)."""
    names = names or glcm_names()
    return np.array([e.value.get(n, np.nan) for n in names])


def row_from_matrices(mats, I, soft_nan=0.0, names=None):
    """A table row computed from (possibly wrong) matrices: what a kernel that counted them would report in the exact columns.  The _AVE
    columns are summed in the order of std::reduce (vol_ref.reduce13), in doubles, as the kernel does."""
    names = names or glcm_names()
    e = from_matrices(mats, I, soft_nan)
    v = {n: x for n, x in e.value.items() if not n.endswith("_AVE")}
    for c in EXACT:
        if c not in gx.NO_AVE:
            v["3GLCM_%s_AVE" % c] = vol_ref.reduce13([e.value["3GLCM_%s_%d" % (c, d)] for d in range(N_DIR)])
    return np.array([v.get(n, np.nan) for n in names])


def compare_vol_exact(got_row, exact: VolExact, Ng, names, ratios=None, tag="", scale=1.0):
    """Mismatches (list of strings, empty = within the bound) of one table row against exact_row's result: compare_glcm_exact's contract
    on the 3-D names.  Ng: the matrix order the tolerance is sized by (exact.Ng; stated by the caller so a test can see it); names: the
    table's column names; ratios: optional dict column -> worst |err| / (2^-53 magnitude) seen, updated in place (the non-scaling part of
    an _AVE tolerance is taken off the error first); scale: a factor on K, never above 1."""
    assert scale <= 1.0
    assert Ng == exact.Ng, (Ng, exact.Ng)
    bad = []
    pos = {n: j for j, n in enumerate(names)}
    for n, want in exact.value.items():
        if n not in pos:
            bad.append(f"{tag}{n}: column missing from the table")
            continue
        g = float(got_row[pos[n]])
        if n in exact.bits:
            if not gx._same_bits(g, want):
                bad.append(f"{tag}{n}: got {g!r}, want {want!r} by bits")
            continue
        mag = exact.magnitude[n]
        extra = exact.ave_round.get(n, 0.0)
        tol = scale * (exact.tol[n] - extra) + extra
        err = abs(g - want)
        if ratios is not None and mag > 0 and math.isfinite(err):
            base = n[6:].rsplit("_", 1)[0] + ("_AVE" if n.endswith("_AVE") else "")
            ratios[base] = max(ratios.get(base, 0.0), max(0.0, err - extra) / (EPS * mag))
        if not err <= tol:                               # (NaN fails)
            bad.append(f"{tag}{n}: got {g!r}, exact {want!r}, |err| {err:.3e} = {err / (EPS * mag) if mag else math.inf:.1f} x 2^-53 magnitude, "
                       f"allowed {scale:g} x K = {scale * K(Ng):g}")
    return bad


def compare_table(G, rows, names, ratios=None, tag="", scale=1.0):
    bad = []
    for r, e in enumerate(rows):
        bad += compare_vol_exact(G[r], e, e.Ng, names, ratios=ratios, tag="%sroi %d " % (tag, r), scale=scale)
    return bad


def sensitivity(exact: VolExact):
    """(drop, move) as glcm_exact_ref.sensitivity defines them, over the 13 directions, from the exact values alone: how many times the
    comparator's tolerance a lost or doubled pair, and a pair moved to another cell, is.  inf for rows without pairs (those compare by
    bits); a direction whose matrix has one occupied cell is left out of `drop` (every normalised column of such a matrix is the same
    for any count)."""
    return gx.sensitivity(exact)
