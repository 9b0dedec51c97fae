"""The integer counts of tests/counts.py on the CPU checkers alone (no GPU, no HIP library): counts worked out by hand, the oracle
against the reference's own classes, and proof that a one-run / one-zone / one-pixel change -- which moves every texture column by
less than the 1e-5 of compare_tables on large ROIs -- is flagged for every family."""
import numpy as np
import pytest

from nyxus_amd import _abi
from oracle import pyoracle as po
from tests import counts, parity
from tests.test_large_rois_gpu import large_rois
from tests.test_size_classes_gpu import ellipse_roi

ALL = _abi.FAM_GLRLM | _abi.FAM_GLSZM | _abi.FAM_NGTDM | _abi.FAM_GLDZM | _abi.FAM_GLDM | _abi.FAM_NGLDM
NAMES = counts.texture_names(ALL)
FAMILIES = ("GLRLM", "GLSZM", "GLDZM", "GLDM", "NGLDM", "NGTDM")


def box_roi(w, h, f):
    """A full w x h box, column-major like the in-memory workflow, intensity f(x, y)."""
    yy, xx = np.mgrid[0:h, 0:w]
    o = np.lexsort((yy.ravel(), xx.ravel()))
    return dict(x=xx.ravel()[o], y=yy.ravel()[o], inten=np.broadcast_to(f(xx, yy), xx.shape).ravel()[o].astype(np.uint32))


def _counts(rois, gd=64):
    O = po.oracle_featurize(_abi.batch_from_rois(rois), ALL, _abi.default_settings(gd))
    return {k: v for k, (v, _) in counts.recover_counts(O, NAMES).items()}, O


def _is(v, n):
    return abs(v - n) <= counts.INT_TOL


def test_texture_names_follow_the_oracle_layout():
    import ctypes
    s = _abi.default_settings(8)
    for fam in (ALL, _abi.FAM_GLRLM, _abi.FAM_GLSZM | _abi.FAM_NGTDM, _abi.FAM_GLDM | _abi.FAM_NGLDM | _abi.FAM_GLDZM):
        assert po.oracle_lib().nyxo_n_columns(fam, ctypes.byref(s)) == len(counts.texture_names(fam))
    assert NAMES[:4] == ["GLRLM_SRE_0", "GLRLM_SRE_45", "GLRLM_SRE_90", "GLRLM_SRE_135"] and NAMES[64] == "GLRLM_SRE_AVE"


@pytest.mark.parametrize("w,h", [(7, 5), (3, 11), (40, 9), (1, 6)])
def test_constant_rectangles(w, h):
    """A constant ROI is degenerate in the reference (every texture column 0), so two constant w x h rectangles of different levels
    side by side: per rectangle h runs at 0 degrees, w at 90, w + h - 1 on each diagonal, one zone."""
    c, _ = _counts([box_roi(2 * w, h, lambda x, y: np.where(x < w, 100, 300))])
    for a, n in ((0, h), (90, w), (45, w + h - 1), (135, w + h - 1)):
        assert _is(c["GLRLM_%d:runs(GLRLM_GLN_%d)" % (a, a)][0], 2 * n), (a, c)
        assert _is(c["GLRLM_%d:runs(GLRLM_RLN_%d)" % (a, a)][0], 2 * n), (a, c)
        assert _is(c["GLRLM_%d:GLRLM_GLN_%d*N" % (a, a)][0], 2 * n * n)            # two levels of n runs each
    for f, x in (("GLSZM", "GLSZM_GLN"), ("GLSZM", "GLSZM_SZN"), ("GLDZM", "GLDZM_GLNU"), ("GLDZM", "GLDZM_ZDNU")):
        assert _is(c["%s:zones(%s)" % (f, x)][0], 2), (f, c)
    assert _is(c["GLSZM:GLSZM_SZN*N"][0], 4)                                         # both zones have w * h pixels
    for k in ("GLDM:pixels(GLDM_DN)", "NGLDM:pixels(NGLDM_GLNU)", "NGLDM:pixels(NGLDM_DCNU)"):
        assert _is(c[k][0], 2 * w * h), (k, c)
    assert _is(c["GLDM:GLDM_GLN*N"][0], 2 * (w * h) ** 2)


@pytest.mark.parametrize("w,h", [(6, 4), (9, 9), (16, 5)])
def test_two_level_checkerboard(w, h):
    """Every horizontal and vertical run has one pixel, every diagonal is one run, every 4-connected GLDZM zone is one pixel.
    (GLSZM zones follow the reference's zone sweep on a checkerboard, which diagonal neighbours join: pinned against the reference
    below, not by hand.)"""
    c, _ = _counts([box_roi(w, h, lambda x, y: 10 + 90 * ((x + y) % 2))])
    for a, n in ((0, w * h), (90, w * h), (45, w + h - 1), (135, w + h - 1)):
        assert _is(c["GLRLM_%d:runs(GLRLM_RLN_%d)" % (a, a)][0], n), (a, c)
    for a in (0, 90):
        assert _is(c["GLRLM_%d:GLRLM_RLN_%d*N" % (a, a)][0], (w * h) ** 2)           # all w * h runs of length 1
    assert _is(c["GLDZM:zones(GLDZM_GLNU)"][0], w * h) and _is(c["GLDZM:zones(GLDZM_ZDNU)"][0], w * h)
    for k in ("GLDM:pixels(GLDM_DN)", "NGLDM:pixels(NGLDM_GLNU)"):
        assert _is(c[k][0], w * h)


@pytest.mark.parametrize("w,t,n", [(5, 3, 4), (30, 1, 8), (12, 7, 5)])
def test_horizontal_stripes_of_distinct_levels(w, t, n):
    """n stripes of t rows, each its own level: n * t runs at 0 degrees, n * w at 90 (each t long), n * (w + t - 1) on each
    diagonal, n zones of w * t pixels."""
    c, _ = _counts([box_roi(w, n * t, lambda x, y: 100 * (1 + y // t) + 0 * x)])
    for a, m in ((0, n * t), (90, n * w), (45, n * (w + t - 1)), (135, n * (w + t - 1))):
        assert _is(c["GLRLM_%d:runs(GLRLM_GLN_%d)" % (a, a)][0], m), (a, c)
    assert _is(c["GLRLM_90:GLRLM_RLN_90*N"][0], (n * w) ** 2)                       # one run length (t) for all n * w runs
    assert _is(c["GLSZM:zones(GLSZM_SZN)"][0], n) and _is(c["GLSZM:GLSZM_SZN*N"][0], n * n)
    assert _is(c["GLSZM:GLSZM_GLN*N"][0], n)                                          # one zone per level
    assert _is(c["GLDZM:zones(GLDZM_GLNU)"][0], n)
    assert _is(c["GLDM:pixels(GLDM_DN)"][0], n * w * t)


@pytest.mark.skipif(not po.have_ref(), reason="reference classes not built (oracle/_ref/libnyxref.so)")
@pytest.mark.parametrize("gd,ibsi", [(8, 0), (64, 0), (-16, 0), (8, 1)])
def test_oracle_counts_equal_the_reference(gd, ibsi):
    """The oracle's recovered counts are the reference's on the large-ROI shapes of the GPU suite (20 k .. 400 k pixels, holes,
    zeros, constant, blank, a 2000 x 12 strip); NGTDM at the tight bound.  (Radiomics binning: no GLDZM / NGLDM, which the
    library refuses there -- the reference's own GLDZM is all zeros under it.)"""
    s = _abi.default_settings(gd)
    s.ibsi = ibsi
    mask = ALL & ~(_abi.FAM_GLDZM | _abi.FAM_NGLDM) if gd < 0 else ALL
    names = counts.texture_names(mask)
    rois = large_rois(hi=200 if ibsi else 4096)
    degenerate = [4, 5]                                    # the constant and the blank ROI: every texture column 0
    if ibsi:
        del rois[5]                                        # (the reference's NGTDM faults on an all-zero ROI under IBSI)
        degenerate = [4]
    b = _abi.batch_from_rois(rois)
    O = po.oracle_featurize(b, mask, s)
    R = po.ref_featurize(b, mask, s, n_threads=4)
    bad = counts.compare_counts(O, R, names) + counts.compare_tight(O, R, names)
    assert not bad, "\n".join(bad[:20])
    # not vacuous: every family has a checked count on every ROI but the degenerate ones
    rec = counts.recover_counts(R, names)
    fams = {q.split(":")[0] for q in rec}
    assert len(fams) == (6 if gd < 0 else 8) and any(n.startswith("NGTDM_") for n in names)
    for fam in fams:
        cov = np.zeros(len(rois), bool)
        for q, v in rec.items():
            if q.startswith(fam + ":"):
                cov |= counts.applicable(v)
        assert list(np.nonzero(~cov)[0]) == degenerate, (fam, cov)


# ---- detection: one-pixel changes on large ellipses -------------------------------------------------------------------------------
def _family_cols(fam):
    return [j for j, n in enumerate(NAMES) if n.startswith(fam + "_")]


def _changed(roi, kind, rng):
    """(before, after): one pixel one grey level up (grey depth 64 of 1 .. 4095: one level is 64), one interior pixel gone, or two
    adjacent rows of levels A and B (A != B) becoming one level A -- their zones and vertical runs merge."""
    x, y, v = roi["x"].astype(np.int64), roi["y"].astype(np.int64), roi["inten"].astype(np.int64).copy()
    cx, cy = (x.max() + 1) // 2, (y.max() + 1) // 2
    if kind == "level":
        cand = np.nonzero((v >= 64) & (v + 64 < v.max()) & (np.abs(x - cx) < 10) & (np.abs(y - cy) < 10))[0]
        i = int(rng.choice(cand))
        w = v.copy()
        w[i] += 64
        return dict(x=x, y=y, inten=v), dict(x=x, y=y, inten=w)
    if kind == "remove":
        # (matlab binning sends the background to level 1, as it does intensities below 64: the pixel gone must not be one of those)
        near = np.nonzero((np.abs(x - cx) < 10) & (np.abs(y - cy) < 10) & (v >= 64))[0]
        keep = np.ones(len(x), bool)
        keep[int(rng.choice(near))] = False
        return dict(x=x, y=y, inten=v), dict(x=x[keep], y=y[keep], inten=v[keep])
    v[y == cy] = 1000
    v[y == cy + 1] = 1064
    w = v.copy()
    w[y == cy + 1] = 1000
    return dict(x=x, y=y, inten=v), dict(x=x, y=y, inten=w)


@pytest.mark.parametrize("a,b", [(90, 72), (150, 120), (210, 166)])      # 20 k, 56 k, 110 k pixels
@pytest.mark.parametrize("kind", ["level", "remove", "merge"])
def test_one_pixel_changes_are_flagged_for_every_family(a, b, kind):
    rng = np.random.default_rng(a + b)
    before, after = _changed(ellipse_roi(a, b, rng), kind, rng)
    s = _abi.default_settings(64)
    B = po.oracle_featurize(_abi.batch_from_rois([before]), ALL, s)
    A = po.oracle_featurize(_abi.batch_from_rois([after]), ALL, s)
    assert not counts.compare_counts(B, B, NAMES) and not counts.compare_tight(B, B, NAMES)
    missed = []
    for fam in FAMILIES:
        cols = _family_cols(fam)
        names = [NAMES[j] for j in cols]
        if not (counts.compare_counts(A[:, cols], B[:, cols], names) + counts.compare_tight(A[:, cols], B[:, cols], names)):
            rel = np.nanmax(np.abs(A[:, cols] - B[:, cols]) / np.maximum(np.abs(B[:, cols]), 1e-300))
            missed.append(f"{fam} (largest relative change {rel:.2g}, compare_tables: {len(parity.compare_tables(A[:, cols], B[:, cols], names))} flags)")
    assert not missed, missed


def test_vacuity_guard():
    """A batch of 32+ rows whose counts are not integers (here: scaled) cannot pass as 'nothing to check'."""
    rng = np.random.default_rng(5)
    rois = [ellipse_roi(int(r), int(r) - 1, rng) for r in rng.integers(4, 12, 34)]
    O = po.oracle_featurize(_abi.batch_from_rois(rois), ALL, _abi.default_settings(8))
    assert not counts.compare_counts(O, O, NAMES)
    cols = [NAMES.index(n) for n in ("GLSZM_GLN", "GLSZM_SZN")]
    W = O.copy()
    W[:, cols] *= 1.0 + 1e-3                              # N = X / XN and S = X * N are no longer integers anywhere
    bad = counts.compare_counts(W, W, NAMES)
    assert any(m.startswith("GLSZM: ") and "no checkable count" in m for m in bad), bad


def test_a_count_off_by_one_is_reported_and_the_two_routes_must_agree():
    rng = np.random.default_rng(9)
    O = po.oracle_featurize(_abi.batch_from_rois([ellipse_roi(40, 30, rng)]), ALL, _abi.default_settings(8))
    j, jn = NAMES.index("GLSZM_SZN"), NAMES.index("GLSZM_SZNN")
    n = O[0, j] / O[0, jn]
    G = O.copy()
    G[0, jn] = O[0, j] / (n + 1)                          # SZN / SZNN names one zone more than GLN / GLNN
    bad = counts.compare_counts(G, O, NAMES)
    assert any("GLSZM:zones(GLSZM_SZN)" in m for m in bad) and any("got has zones" in m for m in bad), bad
    T = O.copy()
    T[0, NAMES.index("NGTDM_BUSYNESS")] *= 1 + 1e-9
    assert counts.compare_tight(T, O, NAMES) and not counts.compare_tight(O, O, NAMES)
