"""roi_vol.hip at its own seams (tests/vol_edge_cases.py).

The GLCM groups run through volumes_host with VFAM_GLCM and with VFAM_ALL and are held to exact rational values
(tests/vol_exact_ref.py): |got - exact| <= (Ng^2 + 2 Ng + 64) 2^-53 magnitude in 24 of the 30 codes of every direction and their _AVE
twins, blank directions, NaN CORRELATIONs and rows without voxels by bits; the six log columns go through vol_cases.compare against
vol_ref; the GLCM block has equal bits under both masks; one group runs from device memory as well.  The sort, mode and bins groups run
under VFAM_INTENSITY against vol_ref.intensity_rows under vol_cases.compare's policy (parity.EXACT_COLUMNS bit for bit, the rest within
parity.REL_TOL), and MODE, MIN, MAX, MEDIAN and INTEGRATED_INTENSITY also against plain NumPy integers computed here, so that a mistake
the C checker shares cannot hide one in the kernel.  Rows keep their bits across input order, batch order and chunks, and across the
65535-ROI bound of a chunk.

Measured on an MI355X (profiles/vol_glcm_exact_margin.txt, tools/vol_glcm_exact_margin.py --hip): the worst |err| / (K 2^-53 magnitude) of
the HIP path over the recorded and the edge cases is 0.023 (SUMAVERAGE, levels 63..66 under radiomics binning), under either mask; the
bound asserted here is the derived 1.0."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from tests import parity, vol_cases, vol_edge_cases as ve, vol_exact_ref as vx, vol_ref
from tests.vol_device import device_rows

pytestmark = pytest.mark.gpu

N_INT = vol_cases.N_INT
NAMES = vx.glcm_names()
INT_NAMES = vol_cases.column_names()[:N_INT]
GLCM, INTENSITY, ALL = _abi.VFAM_GLCM, _abi.VFAM_INTENSITY, _abi.VFAM_ALL


def same(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def vol_ctx():
    """A context of this module's own on cuda:0: the workspaces these entries grow stay out of the context the other test files share."""
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


# ---- GLCM groups ------------------------------------------------------------------------------------------------------------

def check_glcm(G, c, what):
    rows = ve.exact(c)
    worst = (0.0, "")
    bad = []
    for r, e in enumerate(rows):
        ratios = {}
        bad += vx.compare_vol_exact(G[r], e, e.Ng, NAMES, ratios=ratios, tag="roi %d " % r, scale=1.0)
        worst = max([worst] + [(v / vx.K(e.Ng), "%s roi %d Ng %d" % (col, r, e.Ng)) for col, v in ratios.items()])
    print("%s %s: worst |err| / (K 2^-53 magnitude) %.4f (%s)" % (c.id, what, worst[0], worst[1]))
    assert not bad, "%s %s against the exact values:\n%s" % (c.id, what, "\n".join(bad[:20]))
    bad, _, rg = vol_cases.compare(G, ve.reference(c), NAMES)                # the log columns (and every other one at 1e-5, as before)
    assert not bad, "%s %s against vol_ref:\n%s" % (c.id, what, "\n".join(bad[:20]))


def run_case(ctx, c):
    b, s = ve.batch(c.bname), ve.settings(c.mode)
    G = ctx.volumes_host(b, GLCM, s)
    assert G.shape == (b.n_roi, len(NAMES)) and _lib.vol_column_names(GLCM, s) == NAMES
    check_glcm(G, c, "GLCM alone")
    A = ctx.volumes_host(b, ALL, s)
    ok = same(A[:, N_INT:], G)
    assert ok.all(), (c.id, "the GLCM block differs beside the intensity block", [NAMES[j] for j in np.flatnonzero(~ok.all(axis=0))][:8])
    return G


def _cases(g):
    return pytest.mark.parametrize("c", ve.of_group(g), ids=lambda c: c.id)


@_cases("widths")
def test_lane_sharing_widths(vol_ctx, c):
    G = run_case(vol_ctx, c)
    if c == ve.DEVICE_CASE:                                                  # ... and from device memory
        b, s = ve.batch(c.bname), ve.settings(c.mode)
        assert same(device_rows(vol_ctx, b, s, GLCM), G).all()
        assert same(device_rows(vol_ctx, b, s, GLCM, stated=False), G).all()
        assert same(device_rows(vol_ctx, b, s, ALL)[:, N_INT:], G).all()


@_cases("rows")
def test_rows_around_the_row_loops_stride(vol_ctx, c):
    run_case(vol_ctx, c)


@_cases("negshift")
def test_negative_shifts_at_both_borders(vol_ctx, c):
    run_case(vol_ctx, c)


@_cases("tail")
def test_tail_words_of_the_box(vol_ctx, c):
    run_case(vol_ctx, c)


@_cases("levels")
def test_level_sets_across_the_presence_map(vol_ctx, c):
    run_case(vol_ctx, c)


@_cases("offsets")
def test_offsets_up_to_and_beyond_the_box(vol_ctx, c):
    G = run_case(vol_ctx, c)
    blank = [a.blank for a in ve.exact(c)[0].angles]
    T = G[0, :390].reshape(30, 13)
    assert [bool((T[:, d] == 0.0).all()) for d in range(13)] == blank        # (soft_nan = 0: a blank direction is 30 zeros)


@_cases("needles")
def test_needles(vol_ctx, c):
    run_case(vol_ctx, c)


@_cases("seam")
def test_lds_staging_seam(vol_ctx, c):
    run_case(vol_ctx, c)


# ---- intensity groups -------------------------------------------------------------------------------------------------------

def numpy_integers(b, r):
    """(MODE, MIN, MAX, MEDIAN, INTEGRATED_INTENSITY) of row r from np.sort, np.unique and Python integers.  MEDIAN of an even count is the
    mean of the two middle values with their sum taken in 32 bits, as the reference's class takes it (histogram.h:268-287)."""
    v = np.sort(b.inten[int(b.px_offset[r]):int(b.px_offset[r + 1])])
    n = len(v)
    u, cnt = np.unique(v, return_counts=True)
    mode = int(u[np.flatnonzero(cnt == cnt.max())[0]])                       # the smallest value among the most frequent
    med = float(int(v[n // 2])) if n & 1 else ((int(v[n // 2]) + int(v[n // 2 - 1])) & 0xFFFFFFFF) / 2.0
    return float(mode), float(int(v[0])), float(int(v[-1])), med, float(sum(int(x) for x in v))


def check_intensity(ctx, b, s, what):
    got = ctx.volumes_host(b, INTENSITY, s)
    want = vol_ref.intensity_rows(b, s)
    bad, ri, _ = vol_cases.compare(got, want, INT_NAMES)
    print("%s: largest relative difference of the intensity block %.3e" % (what, ri))
    assert not bad, "%s against vol_ref.intensity_rows:\n%s" % (what, "\n".join(bad[:20]))
    cols = [INT_NAMES.index("3" + n) for n in ("MODE", "MIN", "MAX", "MEDIAN", "INTEGRATED_INTENSITY")]
    for r in range(b.n_roi):
        mine = numpy_integers(b, r)
        assert tuple(got[r, cols]) == mine, (what, r, int(b.counts()[r]), list(zip(("MODE", "MIN", "MAX", "MEDIAN", "INTEGRATED_INTENSITY"), got[r, cols], mine)))
    return got


def test_the_order_statistics_compare_by_bits():
    assert {"MODE", "MEDIAN", "MIN", "MAX", "INTEGRATED_INTENSITY", "P01", "P10", "P25", "P75", "P90", "P99"} <= parity.EXACT_COLUMNS


def test_sort_sizes_and_pass_counts(vol_ctx):
    b, s = ve.batch("sort"), _abi.default_settings(64)
    got = check_intensity(vol_ctx, b, s, "sort")
    assert same(got[0::2], got[1::2]).all(), "ascending and descending copies of an ROI"
    order = list(range(b.n_roi))[::-1]
    assert same(vol_ctx.volumes_host(b.select(order), INTENSITY, s)[::-1], got).all(), "the batch reversed"
    one_roi = 8 * ((4 * int(b.counts().max()) + 255) // 256 * 256 // 4)      # two key buffers of the largest ROI, 256-aligned: one ROI a chunk
    assert same(vol_ctx.volumes_host(b, INTENSITY, s, max_device_bytes=one_roi), got).all(), "one ROI a chunk"
    check_intensity(vol_ctx, ve.batch("sort4097"), s, "sort4097")


def test_mode_run_layouts(vol_ctx):
    b, s = ve.batch("mode"), _abi.default_settings(64)
    got = check_intensity(vol_ctx, b, s, "mode")
    j = INT_NAMES.index("3MODE")
    for r, (name, (lengths, mode_run)) in enumerate(ve.MODE_LAYOUTS.items()):
        assert got[r, j] == 10 + 3 * mode_run, (name, got[r, j], 10 + 3 * mode_run)


def test_histogram_bin_counts_up_to_the_cap(vol_ctx):
    b = ve.batch("sort").select(ve.BINS_ROIS)
    for g in ve.BINS_DEPTHS:
        s = _abi.default_settings(64)
        s.grey_depth = g
        check_intensity(vol_ctx, b, s, "bins grey_depth %d" % g)
    for g in ve.BINS_REFUSED:
        s = _abi.default_settings(64)
        s.grey_depth = g
        with pytest.raises(_lib.NyxHipError, match="16384") as ei:
            vol_ctx.volumes_host(b, INTENSITY, s)
        assert ei.value.code == 4                                            # NYXHIP_ERR_UNSUPPORTED
        vol_ctx.volumes_host(ve.batch("boxes"), GLCM, s)                     # the GLCM block does not read the setting
    check_intensity(vol_ctx, b, _abi.default_settings(64), "bins, the call after the refusals")   # the context serves the next call


# ---- the chunk bound --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", [INTENSITY, GLCM], ids=["intensity", "glcm"])
def test_rows_beyond_the_chunk_bound(vol_ctx, mask):
    """65535 + 15 ROIs (the 12 of `boxes`, tiled) under matlab binning: every row has the bits of its pattern's row from the 12-ROI call,
    on both sides of the 65535-ROI bound of a chunk, and rows 65534, 65535 and 65536 are held to the reference as well."""
    p, b, s = ve.batch("boxes"), ve.batch("chunk"), vol_cases.settings("matlab")
    pat = vol_ctx.volumes_host(p, mask, s)
    got = vol_ctx.volumes_host(b, mask, s)
    assert got.shape[0] == ve.CHUNK_ROIS
    ok = same(got, pat[np.arange(b.n_roi) % p.n_roi]).all(axis=1)
    assert ok.all(), np.flatnonzero(~ok)[:10]
    tail = b.select([65534, 65535, 65536])
    if mask == GLCM:
        bad = vx.compare_table(got[65534:65537], vx.exact_rows(tail, s), NAMES)
        bad += vol_cases.compare(got[65534:65537], vol_ref.glcm_rows(tail, s), NAMES)[0]
    else:
        bad = vol_cases.compare(got[65534:65537], vol_ref.intensity_rows(tail, s), INT_NAMES)[0]
    assert not bad, "\n".join(bad[:20])
