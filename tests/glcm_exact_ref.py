"""Exact reference for the GLCM columns, and the comparator that holds a table to it (CPU only; loads no HIP library).

With integer grey levels 24 of the 30 angled GLCM columns are rational functions of the integer co-occurrence matrix (CORRELATION
needs two square roots on top).  This module forms the matrix in integers from a HostBatch row the way glcm_cooc of
oracle/nyx_oracle.c does, evaluates every such column exactly (Python integers over the matrix's one-dimensional marginals, one
correctly rounded int / int at the end; mpmath at 50 digits for CORRELATION), and compare_glcm_exact grants a table

    |got - exact| <= K(Ng) * 2^-53 * magnitude,      K(Ng) = Ng^2 + 2 Ng + 64,

the forward error bound of summing at most Ng^2 cells (or 2 Ng marginal entries) in ANY order, each term with a handful of
roundings of its own; `magnitude` is the sum of the |terms| of the oracle's formula (every subtraction inside a term kept, only
the outer sum made absolute).  K is derived, not measured: a kernel that evaluates an algebraically different form gets that
form's own sum of |terms| added to the column's magnitude (no kernel needed it), never a larger K.  One extension of the magnitude
holds for every implementation, the oracle included: a centred term (v - mu)^k p also carries the rounding of mu itself -- 2^-53 |mu|
absolute however small v - mu is -- which moves it by k |v - mu|^(k-1) |mu| p 2^-53.  On almost flat ROIs (|mu| >> |v - mu|) that
is the larger part (the oracle's JVAR: 27 units of the plain sum at K / 4 = 18), so VARIANCE, JVAR, DIFVAR, CLUTEND, SUMVARIANCE,
CLUSHADE, CLUPROM and CORRELATION count it among their |terms| (exact_angle).  _AVE columns: the mean of
the angle tolerances plus 4 * 2^-53 * |value|.  NaN, soft_nan and 0.0 rows compare by bits.

A lost, doubled or misplaced pair moves JAVE / SUMAVERAGE / CONTRAST / ACOR / DIS by about 1 / N of their value (N counted
pairs): sensitivity() computes, from the exact reference alone, how many times the tolerance that move is, and the tests assert
at least 1000 for every case.

Left out: ENTROPY, JE, SUMENTROPY, DIFENTRO, INFOMEAS1, INFOMEAS2.  They go through fast_log10, a float quadratic on
(float)(p + 1e-9); one ulp in p can flip the float rounding, so no tight bound holds independently of how p was formed.  They
stay on parity.compare_tables (1e-5).

Quirks of the oracle's formulas kept on purpose (nyx_oracle.c:501-833): JVAR weighs the COLUMN marginal with (x + 1) - JAVE;
by_row_mean is the column mean; kSum[s] / kDiff[k] hold the last pair written in loop order (x = min(s, Ng - 1) resp. x = Ng - 1:
this matters under radiomics binning, where the level values are not 1..Ng); the Ng-fold repeat of DIFVAR cancels; DIS weighs
index differences, DIFAVE weighs kDiff.
"""
from __future__ import annotations

import math
from fractions import Fraction

import mpmath
import numpy as np

EPS = 2.0 ** -53
ANGLED = ("ASM", "ACOR", "CLUPROM", "CLUSHADE", "CLUTEND", "CONTRAST", "CORRELATION", "DIFAVE", "DIFENTRO", "DIFVAR", "DIS", "ENERGY",
          "ENTROPY", "HOM1", "HOM2", "ID", "IDN", "IDM", "IDMN", "INFOMEAS1", "INFOMEAS2", "IV", "JAVE", "JE", "JMAX", "JVAR",
          "SUMAVERAGE", "SUMENTROPY", "SUMVARIANCE", "VARIANCE")
LOG_COLUMNS = ("ENTROPY", "JE", "SUMENTROPY", "DIFENTRO", "INFOMEAS1", "INFOMEAS2")
EXACT = tuple(c for c in ANGLED if c not in LOG_COLUMNS)
NO_AVE = ("HOM2",)                                    # the one angled column without an _AVE twin
SENSITIVE = ("JAVE", "SUMAVERAGE", "CONTRAST", "ACOR", "DIS")
_SHIFT = 320                                          # bits kept of the quotients whose common denominator would be lcm(1 + k^2 ...)
_DXDY = {0: (1, 0), 45: (1, 1), 90: (0, 1), 135: (-1, 1)}


def K(Ng: int) -> int:
    return Ng * Ng + 2 * Ng + 64


# ---- binning: texture_feature.h as nyx_oracle.c:346-383 states it, the same double operations in the same order --------------------

def _bin_matlab(x, mx, n):
    x = np.asarray(x, np.uint32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        slope = np.float64(n) / (np.float64(mx) - 0.0)
        intercept = 1.0 - slope * 0.0
        sc = np.floor(slope * x.astype(np.float64) + intercept)
        sc = np.where(np.isfinite(sc), sc, 1.0)       # (mx == 0: only x == 0 reaches the cast in C; every such x is 1 below)
        sc = np.clip(sc, 1.0, float(n)).astype(np.uint32)
    return np.where(x == 0, np.uint32(1), sc).astype(np.uint32)


def _bin_radiomix(x, mn, mx, n):
    x = np.asarray(x, np.uint32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        binw = np.float64(np.uint32(mx) - np.uint32(mn)) / np.float64(n)
        y = (x - np.uint32(mn)).astype(np.float64) / binw + 1     # x - mn wraps as uint32 does in C
        y = np.where(np.isfinite(y), y, float(n))                   # (binw == 0 is undefined in C: the degenerate guard catches mn == mx)
        y = np.minimum(np.floor(y), 4294967295.0).astype(np.uint64)
    y = np.minimum(y, np.uint64(n)).astype(np.uint32)
    return np.where(x == 0, np.uint32(0), y).astype(np.uint32)


def bin_pixels(x, mn, mx, grey_info):
    """nyxo_bin_pixel on an array."""
    if grey_info < 0:
        return _bin_radiomix(x, mn, mx, -grey_info)
    if grey_info > 0:
        return _bin_matlab(x, mx, grey_info)
    return np.asarray(x, np.uint32).copy()


def dense_plane(b, r):
    """nyxo_dense_from_cloud: the ROI's box as a plane, 0 = background, later cloud entries overwrite earlier ones."""
    o0, o1 = int(b.px_offset[r]), int(b.px_offset[r + 1])
    w, h = int(b.bbox_w[r]), int(b.bbox_h[r])
    plane = np.zeros(h * w, np.uint32)
    flat = b.y[o0:o1].astype(np.int64) * w + b.x[o0:o1].astype(np.int64)
    # explicit "last one wins": the last occurrence of every position
    _, first_of_reversed = np.unique(flat[::-1], return_index=True)
    last = len(flat) - 1 - first_of_reversed
    plane[flat[last]] = b.inten[o0:o1][last]
    return plane.reshape(h, w)


# ---- the integer matrix ---------------------------------------------------------------------------------------------------

def levels_of(plane, mn, mx, s):
    """(level index plane, -1 = not counted; level values I; grey_info) as glcm_cooc derives them."""
    grey_info = 0 if s.ibsi else int(s.grey_depth)
    D = bin_pixels(plane, mn, mx, grey_info)
    if grey_info < 0:
        I = np.unique(D[D != 0]).astype(np.int64)
        idx = np.searchsorted(I, D).astype(np.int64)
        idx[D == 0] = -1
    elif grey_info > 0:
        I = np.arange(1, grey_info + 1, dtype=np.int64)
        idx = D.astype(np.int64) - 1
    else:
        I = np.arange(1, int(D.max()) + 1 if D.size else 1, dtype=np.int64)
        idx = D.astype(np.int64) - 1
    idx[plane == 0] = -1                               # a pair is skipped when either ORIGINAL intensity is 0
    return idx, I, grey_info


def cooc_matrix(idx, Ng, dx, dy, symmetric):
    """M[row = centre level, column = neighbour level] in int64 (glcm_cooc: PXY(a, b) with a the neighbour's, b the centre's level)."""
    h, w = idx.shape
    M = np.zeros((Ng, Ng), np.int64)
    if dy >= h or abs(dx) >= w or Ng == 0:
        return M
    ctr = idx[0:h - dy, max(0, -dx):w - max(0, dx)]
    nb = idx[dy:h, max(0, dx):w + min(0, dx)]
    ok = (ctr >= 0) & (nb >= 0)
    np.add.at(M, (ctr[ok], nb[ok]), 1)
    return M + M.T if symmetric else M


# ---- exact columns of one angle ---------------------------------------------------------------------------------------------

class Angle:
    """One angle: M (int64 matrix), N (counted pairs, both directions when symmetric), value / magnitude per exact column (floats),
    frac (the exact values as Fractions, CORRELATION as an mpf), blank (no pairs: every column soft_nan)."""


def _bincount_int(key, weight, n):
    out = np.zeros(n, np.int64)
    np.add.at(out, key, weight)
    return out


def _q(terms):
    """sum of n / d over (n, d) integer pairs, as a Fraction good to 2^-_SHIFT of the largest term (positive terms only)."""
    return Fraction(sum((int(n) << _SHIFT) // int(d) for n, d in terms), 1 << _SHIFT)


def exact_angle(M, I, soft_nan):
    a = Angle()
    a.M = M
    Ng = len(I)
    N = int(M.sum())
    a.N = N
    a.blank = N == 0
    a.value, a.magnitude, a.frac = {}, {}, {}
    if a.blank:
        for c in EXACT:
            a.value[c] = float(soft_nan)
            a.magnitude[c] = 0.0
            a.frac[c] = mpmath.mpf(float(soft_nan)) if c == "CORRELATION" else Fraction(float(soft_nan)) if math.isfinite(soft_nan) else None
        a.bits = set(EXACT)
        return a
    a.bits = set()
    rr, cc = np.nonzero(M)
    m = M[rr, cc]                                       # the occupied cells, int64
    Ir, Ic = I[rr], I[cc]
    rows = [int(v) for v in M.sum(axis=1)]
    cols = [int(v) for v in M.sum(axis=0)]
    Il = [int(v) for v in I]
    Dk = [int(v) for v in _bincount_int(np.abs(rr - cc), m, Ng)]               # N * Pxmy[k], by index difference
    Sk = [int(v) for v in _bincount_int(rr + cc, m, 2 * Ng)]                   # N * Pxpy[k], by index sum
    smax = 2 * Il[-1] + 1
    Sv = [int(v) for v in _bincount_int(Ir + Ic, m, smax)]                     # counts by VALUE sum (the cluster columns)
    Dv = [int(v) for v in _bincount_int(np.abs(Ir - Ic), m, Il[-1] + 1)]       # counts by VALUE difference (CONTRAST)
    kSum = [Il[min(k, Ng - 1)] + Il[k - min(k, Ng - 1)] if k <= 2 * Ng - 2 else 0 for k in range(2 * Ng)]
    kDiff = [abs(Il[Ng - 1] - Il[Ng - 1 - k]) for k in range(Ng)]
    Ar = sum(n * v for n, v in zip(rows, Il))           # N * row mean  (JAVE, VARIANCE, CORRELATION's mr)
    Ac = sum(n * v for n, v in zip(cols, Il))           # N * column mean (by_row_mean, CORRELATION's mc)
    R2 = sum(n * v * v for n, v in zip(rows, Il))
    C2 = sum(n * v * v for n, v in zip(cols, Il))
    ACn = sum(int(v) for v in (m * Ir * Ic).tolist())   # (int64 products: counts < 2^31, levels < 2^16 in every case this serves)
    assert int(m.max()) * Il[-1] * Il[-1] < 2 ** 62
    F = Fraction
    fr = a.frac
    fr["ASM"] = fr["ENERGY"] = F(sum(v * v for v in m.tolist()), N * N)
    fr["ACOR"] = F(ACn, N)
    fr["CONTRAST"] = F(sum(n * d * d for d, n in enumerate(Dv)), N)
    fr["DIS"] = F(sum(n * k for k, n in enumerate(Dk)), N)
    DA = sum(n * kDiff[k] for k, n in enumerate(Dk))
    fr["DIFAVE"] = F(DA, N)
    fr["DIFVAR"] = F(sum(n * (N * k - DA) ** 2 for k, n in enumerate(Dk)), N ** 3)
    fr["JAVE"] = F(Ar, N)
    fr["JMAX"] = F(int(m.max()), N)
    fr["JVAR"] = F(sum(n * (N * (x + 1) - Ar) ** 2 for x, n in enumerate(cols)), N ** 3)
    fr["VARIANCE"] = F(N * R2 - Ar * Ar, N * N)
    fr["SUMAVERAGE"] = F(sum(n * kSum[k] for k, n in enumerate(Sk)), N)
    occ_s = [(sv, n) for sv, n in enumerate(Sv) if n]
    fr["CLUTEND"] = fr["SUMVARIANCE"] = F(sum(n * (N * sv - 2 * Ac) ** 2 for sv, n in occ_s), N ** 3)
    fr["CLUSHADE"] = F(sum(n * (N * sv - 2 * Ac) ** 3 for sv, n in occ_s), N ** 4)
    fr["CLUPROM"] = F(sum(n * (N * sv - 2 * Ac) ** 4 for sv, n in occ_s), N ** 5)
    occ_k = [(k, n) for k, n in enumerate(Dk) if n]
    fr["HOM1"] = fr["ID"] = _q((n, N * (1 + k)) for k, n in occ_k)
    fr["HOM2"] = fr["IDM"] = _q((n, N * (1 + k * k)) for k, n in occ_k)
    fr["IDN"] = _q((n * Ng, N * (Ng + k)) for k, n in occ_k)
    fr["IDMN"] = _q((n * Ng * Ng, N * (Ng * Ng + k * k)) for k, n in occ_k)
    fr["IV"] = _q((n, N * kDiff[k] * kDiff[k]) for k, n in occ_k if k >= 1)
    for c, v in fr.items():
        a.value[c] = v.numerator / v.denominator        # int / int: one correctly rounded step
        a.magnitude[c] = abs(a.value[c])                # sums of positive terms; the two cancelling columns follow
    mu2 = 2.0 * Ac / N
    a.magnitude["CLUSHADE"] = float(sum(n * abs(sv - mu2) ** 3 for sv, n in occ_s)) / N
    # the centred columns: a term (v - mu)^k p carries the rounding of mu itself, 2^-53 |mu| absolute whatever |v - mu| is, which
    # moves the term by k |v - mu|^(k-1) |mu| p 2^-53 -- part of the form's own sum of |terms| (almost flat ROIs: |mu| >> |v - mu|)
    # (second order, seen only where the first vanishes -- all mass on one difference k = DIFAVE gives DIFVAR = 0 exactly and
    #  (2^-53 |mu|)^2-sized values from any implementation that rounds mu: the term |mu|^k (K 2^-53)^(k-1), far below everything else)
    jave, da, ke = Ar / N, DA / N, K(Ng) * EPS
    a.magnitude["JVAR"] += 2 * abs(jave) * float(sum(n * abs(x + 1 - jave) for x, n in enumerate(cols))) / N + ke * jave ** 2
    a.magnitude["VARIANCE"] += 2 * abs(jave) * float(sum(n * abs(v - jave) for v, n in zip(Il, rows))) / N + ke * jave ** 2
    a.magnitude["DIFVAR"] += 2 * abs(da) * float(sum(n * abs(k - da) for k, n in occ_k)) / N + ke * da ** 2
    for c, p in (("CLUTEND", 2), ("SUMVARIANCE", 2), ("CLUSHADE", 3), ("CLUPROM", 4)):
        a.magnitude[c] += p * abs(mu2) * float(sum(n * abs(sv - mu2) ** (p - 1) for sv, n in occ_s)) / N + ke ** (p - 1) * abs(mu2) ** p
    # CORRELATION = (N ACn - Ar Ac) / sqrt((N R2 - Ar^2) (N C2 - Ac^2)); a zero denominator is soft_nan by bits
    Vr, Vc = N * R2 - Ar * Ar, N * C2 - Ac * Ac
    if Vr * Vc == 0:
        a.value["CORRELATION"], a.magnitude["CORRELATION"] = float(soft_nan), 0.0
        fr["CORRELATION"] = mpmath.mpf(float(soft_nan))
        a.bits.add("CORRELATION")
    else:
        with mpmath.workprec(200):
            v = mpmath.mpf(N * ACn - Ar * Ac) / mpmath.sqrt(mpmath.mpf(Vr * Vc))
            fr["CORRELATION"] = v
            a.value["CORRELATION"] = float(v)
        sr, sc = math.sqrt(Vr) / N, math.sqrt(Vc) / N
        t = np.abs(Ir - Ar / N) * np.abs(Ic - Ac / N) * m
        a.magnitude["CORRELATION"] = float(t.sum()) / N / (sr * sc) + abs(a.value["CORRELATION"])
        # ... and the roundings of the two means, through the products and through the two deviations
        mr, mc = Ar / N, Ac / N
        dr, dc = float((np.abs(Ir - mr) * m).sum()) / N, float((np.abs(Ic - mc) * m).sum()) / N
        a.magnitude["CORRELATION"] += (abs(mr) * dc + abs(mc) * dr) / (sr * sc) + abs(a.value["CORRELATION"]) * (abs(mr) * dr / sr ** 2 + abs(mc) * dc / sc ** 2)
    return a


class GlcmExact:
    """One ROI under one Settings.  degenerate: the whole row is 0.0 (nyxo_glcm's guard).  Ng: matrix order.  angles: list of Angle
    in request order.  value / tol / bits: per column NAME of the table ('GLCM_ASM_45', 'GLCM_ASM_AVE', ...) the expected double,
    the tolerance, and whether the column compares by bits."""


def exact_glcm(b, r, s) -> GlcmExact:
    """The exact GLCM columns of row r of HostBatch b under Settings s."""
    e = GlcmExact()
    na = int(s.glcm_n_angles)
    angles = [int(s.glcm_angles[i]) for i in range(na)]
    mn, mx = int(b.min_inten[r]), int(b.max_inten[r])
    soft_nan = float(s.soft_nan)
    e.value, e.tol, e.bits, e.magnitude, e.angles, e.request = {}, {}, set(), {}, [], angles
    names = ["GLCM_%s_%d" % (c, a) for c in EXACT for a in angles] + ["GLCM_%s_AVE" % c for c in EXACT if c not in NO_AVE]
    gd = int(s.glcm_grey_depth)                          # the guard bins with glcm_grey_depth, IBSI or not (nyx_oracle.c:855-856)
    e.degenerate = int(bin_pixels([mn], mn, mx, gd)[0]) == int(bin_pixels([mx], mn, mx, gd)[0])
    if e.degenerate:
        e.Ng = 0
        for n in names:
            e.value[n], e.tol[n], e.magnitude[n] = 0.0, 0.0, 0.0
        e.bits = set(names)
        return e
    plane = dense_plane(b, r)
    idx, I, grey_info = levels_of(plane, mn, mx, s)
    e.Ng = Ng = len(I)
    sym = bool(s.glcm_symmetric) or grey_info <= 0
    off = int(s.glcm_offset)
    for ang in angles:
        dx, dy = _DXDY[ang]
        e.angles.append(exact_angle(cooc_matrix(idx, Ng, dx * off, dy * off, sym), I, soft_nan))
    k = K(Ng)
    for c in EXACT:
        for ang, a in zip(angles, e.angles):
            n = "GLCM_%s_%d" % (c, ang)
            e.value[n], e.magnitude[n], e.tol[n] = a.value[c], a.magnitude[c], k * EPS * a.magnitude[c]
            if c in a.bits:
                e.bits.add(n)
        if c in NO_AVE or na == 0:
            continue
        n = "GLCM_%s_AVE" % c
        if c == "CORRELATION":
            with mpmath.workprec(200):
                v = float(sum(a.frac[c] for a in e.angles) / na)
        else:
            v = sum(a.frac[c] for a in e.angles) / na
            v = v.numerator / v.denominator
        e.value[n] = v
        e.magnitude[n] = sum(a.magnitude[c] for a in e.angles) / na
        e.tol[n] = k * EPS * e.magnitude[n] + 4 * EPS * abs(v)
        if all(c in a.bits for a in e.angles):          # every angle soft_nan: the mean of equal values is that value
            e.bits.add(n)
    return e


def table_row(e: GlcmExact, names):
    """The exact columns of e laid out as a table row under `names` (NaN where the reference has no value: log columns, other families)."""
    return np.array([e.value.get(n, np.nan) for n in names])


def row_from_matrices(mats, I, angles, names, soft_nan=0.0):
    """A table row computed from (possibly wrong) matrices: what a kernel that counted them would report in the exact columns."""
    na = len(angles)
    A = [exact_angle(np.asarray(M, np.int64), np.asarray(I, np.int64), soft_nan) for M in mats]
    v = {}
    for c in EXACT:
        for ang, a in zip(angles, A):
            v["GLCM_%s_%d" % (c, ang)] = a.value[c]
        if c not in NO_AVE:
            v["GLCM_%s_AVE" % c] = float(sum(mpmath.mpf(a.value[c]) for a in A) / na)
    return np.array([v.get(n, np.nan) for n in names])


# ---- the comparator ---------------------------------------------------------------------------------------------------------

def _same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (math.isnan(a) and math.isnan(b))


def compare_glcm_exact(got_row, exact: GlcmExact, Ng, names, na, ratios=None, tag="", scale=1.0):
    """Mismatches (list of strings, empty = within the bound) of one table row against exact_glcm's result.  Ng: the matrix order
    the tolerance is sized by (exact.Ng; stated by the caller so a test can see it); names: the table's column names; na: angles
    requested.  ratios: optional dict column -> worst |err| / (2^-53 magnitude) seen, updated in place (margin reports).  scale: a factor
    on K (the CPU test holds the oracle to K / 4; nothing may pass a value above 1)."""
    assert scale <= 1.0
    assert na == len(exact.request), (na, exact.request)
    assert exact.degenerate or Ng == exact.Ng, (Ng, exact.Ng)
    k = K(Ng)
    bad = []
    pos = {n: j for j, n in enumerate(names)}
    for n, want in exact.value.items():
        if n not in pos:
            bad.append(f"{tag}{n}: column missing from the table")
            continue
        g = float(got_row[pos[n]])
        if n in exact.bits:
            if not _same_bits(g, want):
                bad.append(f"{tag}{n}: got {g!r}, want {want!r} by bits")
            continue
        mag = exact.magnitude[n]
        tol = scale * k * EPS * mag + (4 * EPS * abs(want) if n.endswith("_AVE") else 0.0)
        err = abs(g - want)
        if ratios is not None and mag > 0 and math.isfinite(err):
            base = n[5:].rsplit("_", 1)[0]
            ratios[base] = max(ratios.get(base, 0.0), err / (EPS * mag))
        if not err <= tol:                               # (NaN fails)
            bad.append(f"{tag}{n}: got {g!r}, exact {want!r}, |err| {err:.3e} = {err / (EPS * mag) if mag else math.inf:.1f} x 2^-53 magnitude, "
                       f"allowed {scale:g} x K = {scale * k:g}")
    return bad


def sensitivity(exact: GlcmExact):
    """(drop, move): how many times the comparator's tolerance a one-pair error is, the smallest over the angles with pairs of the
    best column's ratio, both sides relative to the column.  drop: a lost or doubled pair moves X = A / N by at least
    dist(X, Z) / (N + 2), X any of SENSITIVE; move: a count moved to another cell moves JAVE or SUMAVERAGE by at least 1 / N.
    Computed from the exact reference alone.  An angle whose matrix has ONE occupied cell is left out of `drop`: every normalised
    column of such a matrix is the same for any count, so no comparator can see a doubled pair there, and losing its last pair
    gives the blank row, which compares by bits.  inf for degenerate rows and rows without pairs (those compare by bits)."""
    k = K(exact.Ng)
    w_drop = w_move = math.inf
    for a in exact.angles:
        if a.blank:
            continue
        drop = move = 0.0
        for c in SENSITIVE:
            X = a.frac[c]
            if X == 0:
                continue
            tol_rel = k * EPS * a.magnitude[c] / abs(a.value[c])
            f = X - math.floor(X)
            drop = max(drop, float(min(f, 1 - f)) / (a.N + 2) / abs(a.value[c]) / tol_rel)
            if c in ("JAVE", "SUMAVERAGE"):
                move = max(move, (1.0 / a.N) / abs(a.value[c]) / tol_rel)
        w_drop, w_move = w_drop if np.count_nonzero(a.M) == 1 else min(w_drop, drop), min(w_move, move)
    return w_drop, w_move
