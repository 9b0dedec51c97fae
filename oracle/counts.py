"""Integer counts recovered from the texture columns: a check that sees one run, zone or pixel out of tens of thousands.

Several texture columns come in pairs X = S / N and XN = S / N^2, where N is a count (runs of one GLRLM direction, zones, pixels)
and S an integer sum of squares of the matrix marginals.  N = X / XN and S = X * N are then integers, and an error in one run, zone
or pixel moves one of them by at least 1 -- a change of 1e-6 relative or less on a large ROI, which the 1e-5 bound of
compare_tables (tests/parity.py) does not see.  compare_counts checks those integers; compare_tight checks NGTDM, which has no such
pair, at a relative bound measured on the large-ROI batches (profiles/r07_parity_margin_large.txt).

It lives beside the oracle rather than under tests/ because the fuzzers of tools/ use it as well; tests/counts.py is the name the
suite imports it by.

Column layouts: GLRLM is feature-major, 16 names x the angles 0 / 45 / 90 / 135, then 16 _AVE columns; the other families follow
nyxus_amd/featureset.py."""
from __future__ import annotations

import numpy as np

from tests.parity import WAIVE_LIMIT

INT_TOL = 1e-6              # distance from an integer below which a recovered quantity of the expected table counts as an integer
# The HIP value X * N carries the rounding of its own X: one ulp of X moves S ~ 1e10 by 2e-6.  It must be an integer to
# max(INT_TOL, INT_REL * |S|) -- 64 ulps, 2e-3 at 1.5e11, far below the 1 a count error moves it by -- and round to the same integer.
INT_REL = 2.0 ** -46
INT_MAX = 2.0 ** 50         # recovered quantities at or beyond this are not checked (X * N loses the units digit)
# NGTDM: 100 x the worst relative difference HIP vs. oracle on the batches of tools/parity_margin.py --large
# (profiles/r07_parity_margin_large.txt: 4.79e-12, NGTDM_STRENGTH at grey depth 4094), at most 1e-9.  At 8 / 64 levels the worst is
# ~1e-14; the difference grows with the level count because CONTRAST / STRENGTH / COMPLEXITY are sums over level pairs (16 M terms at
# 4094 levels) that the kernel and the oracle add in different orders.
NGTDM_REL = 4.8e-10

# family -> (count name, [(numerator X, denominator XN)] giving N = X / XN, [(name of S, X, XN)] giving S = X * (X / XN))
_FAMILIES = {
    "GLSZM": ("zones", [("GLSZM_GLN", "GLSZM_GLNN"), ("GLSZM_SZN", "GLSZM_SZNN")]),
    "GLDZM": ("zones", [("GLDZM_GLNU", "GLDZM_GLNUN"), ("GLDZM_ZDNU", "GLDZM_ZDNUN")]),
    "GLDM": ("pixels", [("GLDM_DN", "GLDM_DNN")]),
    "NGLDM": ("pixels", [("NGLDM_GLNU", "NGLDM_GLNUN"), ("NGLDM_DCNU", "NGLDM_DCNUN")]),
}
for _a in (0, 45, 90, 135):
    _FAMILIES["GLRLM_%d" % _a] = ("runs", [("GLRLM_GLN_%d" % _a, "GLRLM_GLNN_%d" % _a), ("GLRLM_RLN_%d" % _a, "GLRLM_RLNN_%d" % _a)])
# the integer sums S = X * N; GLDM has no GLNN column, its GLN sum takes N from DN / DNN
_SUMS = {
    "GLSZM": [("GLSZM_GLN", None), ("GLSZM_SZN", None)],
    "GLDZM": [("GLDZM_GLNU", None), ("GLDZM_ZDNU", None)],
    "GLDM": [("GLDM_DN", None), ("GLDM_GLN", ("GLDM_DN", "GLDM_DNN"))],
    "NGLDM": [("NGLDM_GLNU", None), ("NGLDM_DCNU", None)],
}
for _a in (0, 45, 90, 135):
    _SUMS["GLRLM_%d" % _a] = [("GLRLM_GLN_%d" % _a, None), ("GLRLM_RLN_%d" % _a, None)]

TIGHT_COLUMNS = ("NGTDM_COARSENESS", "NGTDM_CONTRAST", "NGTDM_BUSYNESS", "NGTDM_COMPLEXITY", "NGTDM_STRENGTH")


def _family_of(key):
    return key.split("_")[0]                  # GLRLM_90 -> GLRLM


def recover_counts(table, names):
    """{quantity: (values per row, denominator column per row)} for every family whose columns are in `names`.  Quantities are named
    '<family>:<count>(<X>)' for N = X / XN and '<family>:<X>*N' for S = X * N."""
    col = {n: j for j, n in enumerate(names)}
    t = np.asarray(table, dtype=np.float64)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for fam, (what, pairs) in _FAMILIES.items():
            if not all(x in col and xn in col for x, xn in pairs):
                continue
            n_of = {}
            for x, xn in pairs:
                X, XN = t[:, col[x]], t[:, col[xn]]
                n_of[x] = X / XN
                out["%s:%s(%s)" % (fam, what, x)] = (n_of[x], XN)
            for x, via in _SUMS[fam]:
                vx, vxn = via if via is not None else (x, dict(pairs)[x])
                XN = t[:, col[vxn]]
                out["%s:%s*N" % (fam, x)] = (t[:, col[x]] * n_of[vx], XN)
    return out


def _near_int(v):
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (np.abs(v - np.rint(v)) <= INT_TOL) & (np.abs(v) < INT_MAX)


def applicable(want_q):
    """Rows where a quantity of the expected table is checked: an integer to INT_TOL, below INT_MAX, non-zero denominator."""
    v, den = want_q
    return _near_int(v) & np.isfinite(den) & (den != 0)


def compare_counts(got, want, names, max_rows=3):
    """Mismatch messages (empty = the counts agree).  Where a quantity applies (see `applicable`), the HIP value must round to the
    expected integer and be an integer itself; the two ways to a family's N must agree in both tables; and on 32 rows or more, a
    family with no applicable quantity on more than WAIVE_LIMIT of its non-degenerate rows is a mismatch (a vacuous check)."""
    assert np.shape(got) == np.shape(want), (np.shape(got), np.shape(want))
    rg, rw = recover_counts(got, names), recover_counts(want, names)
    col = {n: j for j, n in enumerate(names)}
    w_tab = np.asarray(want, dtype=np.float64)
    bad = []
    n_rows = w_tab.shape[0]
    covered = {}
    for q, wq in rw.items():
        fam = q.split(":")[0]
        ok_w = applicable(wq)
        covered[fam] = covered.get(fam, np.zeros(n_rows, bool)) | ok_w
        g, w = rg[q][0], wq[0]
        with np.errstate(invalid="ignore"):
            fine = np.isfinite(g) & (np.rint(g) == np.rint(w)) & (np.abs(g - np.rint(w)) <= np.maximum(INT_TOL, INT_REL * np.abs(w)))
        for i in np.nonzero(ok_w & ~fine)[0][:max_rows]:
            bad.append(f"{q} roi {i}: got {g[i]!r} want {w[i]!r}")
    # the two routes to N (GLN / GLNN and RLN / RLNN, ...) name the same count
    for fam, (what, pairs) in _FAMILIES.items():
        if len(pairs) < 2 or not all(x in col and xn in col for x, xn in pairs):
            continue
        k1, k2 = ("%s:%s(%s)" % (fam, what, x) for x, _ in pairs[:2])
        both = applicable(rw[k1]) & applicable(rw[k2])
        for tag, r in (("want", rw), ("got", rg)):
            a, b = r[k1][0], r[k2][0]
            with np.errstate(invalid="ignore"):
                agree = np.isfinite(a) & np.isfinite(b) & (np.rint(a) == np.rint(b)) & (np.abs(a - np.rint(a)) <= INT_TOL) & (np.abs(b - np.rint(b)) <= INT_TOL)
            for i in np.nonzero(both & ~agree)[0][:max_rows]:
                bad.append(f"{fam} roi {i}: {tag} has {what} {a[i]!r} by {pairs[0][0]} and {b[i]!r} by {pairs[1][0]}")
    # vacuity: rows whose family columns are not all zero / NaN must mostly have something checked
    if n_rows >= 32:
        for fam, cov in covered.items():
            base = _family_of(fam)
            cols = [j for n, j in col.items() if n.startswith(base + "_") and not n.endswith("_AVE")]
            sub = w_tab[:, cols]
            with np.errstate(invalid="ignore"):
                live = (np.isfinite(sub) & (sub != 0)).any(axis=1)
            idle = int((live & ~cov).sum())
            if idle > WAIVE_LIMIT * int(live.sum()):
                bad.append(f"{fam}: {idle} of {int(live.sum())} non-degenerate rows have no checkable count")
    return bad


def compare_tight(got, want, names, rel=None, max_rows=3):
    """NGTDM columns at a relative bound (NGTDM_REL): NaN against NaN and equal infinities agree, anything else must be within
    rel * |want|."""
    rel = NGTDM_REL if rel is None else rel
    bad = []
    for j, name in enumerate(names):
        if name not in TIGHT_COLUMNS:
            continue
        g = np.asarray(got, dtype=np.float64)[:, j]
        w = np.asarray(want, dtype=np.float64)[:, j]
        with np.errstate(invalid="ignore"):
            ok = (np.isnan(g) & np.isnan(w)) | (g == w) | (np.abs(g - w) <= rel * np.abs(w))
        for i in np.nonzero(~ok)[0][:max_rows]:
            bad.append(f"{name} roi {i}: got {g[i]!r} want {w[i]!r} (rel {abs(g[i] - w[i]) / max(abs(w[i]), 1e-300):.3g})")
    return bad


def texture_names(mask):
    """Column names of the texture families of `mask` in the library's order (GLRLM, GLDZM, GLSZM, GLDM, NGLDM, NGTDM), from
    nyxus_amd/featureset.py alone: no HIP library needed."""
    from nyxus_amd import _abi, featureset as fs
    out = []
    if mask & _abi.FAM_GLRLM:
        out += ["%s_%d" % (n, a) for n in fs.GLRLM_ANGLED for a in (0, 45, 90, 135)] + list(fs.GLRLM_AVE)
    for fam, cols in ((_abi.FAM_GLDZM, fs.GLDZM), (_abi.FAM_GLSZM, fs.GLSZM), (_abi.FAM_GLDM, fs.GLDM), (_abi.FAM_NGLDM, fs.NGLDM),
                      (_abi.FAM_NGTDM, fs.NGTDM)):
        if mask & fam:
            out += list(cols)
    return out
