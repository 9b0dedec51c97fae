"""Every form of the co-occurrence sweep against exact rational values (tests/glcm_exact_ref.py) on the cases of
tests/glcm_exact_cases.py: |got - exact| <= (Ng^2 + 2 Ng + 64) 2^-53 magnitude in 24 of the 30 angled columns and their _AVE twins,
where one pair lost at a strip seam, a halo lane or the 63 | 64 column boundary is six orders above the bound.  Every case runs as
GLCM alone and as INTENSITY + GLCM (the builds differ), is compared with the oracle through parity.compare_tables as before (the six
log columns), and asserts from launch_report() what the report can tell about the path the case was written for.

Measured margins of the HIP path: profiles/glcm_exact_margin.txt (tools/glcm_exact_margin.py --hip)."""
import functools

import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import glcm_exact_cases as gc
from tests import glcm_exact_ref as gx
from tests import parity, synth

pytestmark = pytest.mark.gpu

INT, GLCM = _abi.FAM_INTENSITY, _abi.FAM_GLCM
MASKS = (GLCM, INT | GLCM)


def glcm_columns(table, names):
    """The GLCM block of a table."""
    j = [k for k, n in enumerate(names) if n.startswith("GLCM_")]
    return np.ascontiguousarray(table[:, j]), [names[k] for k in j]


@functools.lru_cache(maxsize=None)
def _oracle(i):
    c = gc.CASES[i]
    s = c.settings()
    return po.oracle_featurize(gc.batch(c), GLCM, s), _lib.column_names(GLCM, s)


def check_path(c, rep):
    if c.sizes:
        assert all(r["size_class"] in c.sizes or (r["class"] < 0 and max(c.sizes) <= 1 and r["max_side"] <= 64) for r in rep), rep
    if c.workspace is not None:
        assert any(r["workspace"] & 1 for r in rep) == c.workspace, rep
    if c.coop is not None:
        assert all(bool(r["cooperative"] & 1) == c.coop for r in rep), rep


def check_table(G, names, exact_rows, want, want_names, what, ratios=None):
    bad = []
    for r, e in enumerate(exact_rows):
        bad += gx.compare_glcm_exact(G[r], e, e.Ng, names, len(e.request), ratios=ratios, tag="roi %d " % r)
    assert not bad, "%s against the exact values:\n%s" % (what, "\n".join(bad[:20]))
    g, gn = glcm_columns(G, names)
    assert gn == want_names
    bad = parity.compare_tables(g, want, gn)
    assert not bad, "%s against the oracle:\n%s" % (what, "\n".join(bad[:20]))


def run_case(ctx, c, ratios=None):
    b, s = gc.batch(c), c.settings()
    want, want_names = _oracle(gc.CASES.index(c))
    tables = []
    for mask in MASKS:
        G = ctx.featurize_host(b, mask, s)
        rep = ctx.launch_report()
        check_table(G, _lib.column_names(mask, s), gc.exact(c), want, want_names, "%s mask %d" % (c.id, mask), ratios)
        check_path(c, rep)
        tables.append(G)
    return tables


def _cases(g):
    return pytest.mark.parametrize("c", gc.of_group(g), ids=lambda c: c.id)


@_cases("S")
def test_smallest_class(hip_ctx, c):
    run_case(hip_ctx, c)


@_cases("W")
def test_widths_at_up_to_16_levels(hip_ctx, c):
    run_case(hip_ctx, c)


@_cases("G")
def test_16_bit_cells(hip_ctx, c):
    run_case(hip_ctx, c)


@_cases("D")
def test_deep_matrices(hip_ctx, c):
    run_case(hip_ctx, c)


@_cases("X")
def test_matrices_beyond_lds(hip_ctx, c):
    run_case(hip_ctx, c)


@_cases("L")
def test_large_roi_path(hip_ctx, c):
    run_case(hip_ctx, c)


@pytest.mark.parametrize("c", [c for c in gc.of_group("L") if c.request in ("usual", "sym", "off2")][:5], ids=lambda c: c.id)
def test_large_rows_keep_their_bits_among_small_companions(hip_ctx, c):
    """The rows of the large boxes alone and in one call with the boxes of groups S and W: equal by bits, and the companions' rows
    within the exact bound there too."""
    s = c.settings()
    small = next(x for x in gc.of_group("S") if x.gd == 8)
    wide = next(x for x in gc.of_group("W") if x.name == "widths" and x.gd == 8)
    if c.ibsi:                                                     # (IBSI: the companions' intensities are their levels -- keep them small)
        comp = [dict(r, inten=(1 + np.asarray(r["inten"]) % 60).astype(np.uint32)) for r in gc.rois(small) + gc.rois(wide)]
    else:
        comp = list(gc.rois(small) + gc.rois(wide))
    large = list(gc.rois(c))
    order = [comp[k] for k in range(0, len(comp), 2)] + large + [comp[k] for k in range(1, len(comp), 2)]
    first = len(range(0, len(comp), 2))
    b_mixed, b_alone = _abi.batch_from_rois(order), gc.batch(c)
    for mask in MASKS:
        names = _lib.column_names(mask, s)
        alone = hip_ctx.featurize_host(b_alone, mask, s)
        mixed = hip_ctx.featurize_host(b_mixed, mask, s)
        part = mixed[first:first + len(large)]
        same = (part == alone) | (np.isnan(part) & np.isnan(alone))
        assert same.all(), (c.id, mask, [names[j] for j in np.nonzero(~same.all(axis=0))[0]][:8])
        bad = []
        for r in list(range(first)) + list(range(first + len(large), b_mixed.n_roi)):
            e = gx.exact_glcm(b_mixed, r, s)
            bad += gx.compare_glcm_exact(mixed[r], e, e.Ng, names, len(e.request), tag="roi %d " % r)
        assert not bad, "\n".join(bad[:20])


# ---- T: the other entries ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
def test_dense_loader(hip_ctx, dtype):
    """A 130 x 129 slide through featurize_slides_host (the dense loader; a slide of this size is served with the large ROIs)."""
    img = gc.slide(dtype)
    b = gc.slide_batch(img)
    for gd, req in ((8, "usual"), (64, "sym")):
        s = gc.settings(gd, False, req)
        want = po.oracle_featurize(b, GLCM, s)
        e = gx.exact_glcm(b, 0, s)
        assert min(gx.sensitivity(e)) >= 1000
        for mask in MASKS:
            G = hip_ctx.featurize_slides_host(img[None], mask, s)
            rep = hip_ctx.launch_report()
            assert rep and all(r["cooperative"] & 1 and r["size_class"] >= 3 for r in rep), rep
            check_table(G, _lib.column_names(mask, s), [e], want, _lib.column_names(GLCM, s), "slide %s gd %d %s mask %d" % (dtype.__name__, gd, req, mask))


def test_window_loader(hip_ctx):
    """One 96 x 96 tile with four ROIs through featurize_tiles_host."""
    inten, lab = gc.tile96()
    b = _abi.batch_from_rois(synth.rois_from_tile(inten, lab))
    for gd, req in ((8, "usual"), (64, "a45_135")):
        s = gc.settings(gd, False, req)
        want = po.oracle_featurize(b, GLCM, s)
        ex = [gx.exact_glcm(b, r, s) for r in range(b.n_roi)]
        assert all(min(gx.sensitivity(e)) >= 1000 for e in ex)
        for mask in MASKS:
            tiles, labels, G = hip_ctx.featurize_tiles_host(inten[None], lab[None], mask, s)
            assert list(labels) == [3, 5, 9, 12] and list(tiles) == [0, 0, 0, 0]
            check_table(G, _lib.column_names(mask, s), ex, want, _lib.column_names(GLCM, s), "tile gd %d %s mask %d" % (gd, req, mask))
