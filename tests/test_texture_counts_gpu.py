"""The texture families on large ROIs at the integer counts of tests/counts.py: one run split or joined at a strip seam, one zone cut
in two, one pixel in the wrong level is a mismatch here, where compare_tables (1e-5 relative) cannot see it on tens of thousands of
runs.  The ROIs walk what roi_large_tex.hip does: strips of kLtexCells / w rows (1, 2, 3, 63, 64, 65 rows; k strips and k +- 1 rows),
runs and zones that cross every seam, holes on seam rows; the boxes where the launch changes form (size class 2, widths around a
wave, a box too wide for the strip kernels); and the GLDZM / GLDM / NGLDM chain of roi_dependence.hip on big boxes."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import counts, parity
from tests.test_size_classes_gpu import ellipse_roi

pytestmark = pytest.mark.gpu

TEX = _abi.FAM_GLRLM | _abi.FAM_GLSZM | _abi.FAM_NGTDM
DEP = _abi.FAM_GLDZM | _abi.FAM_GLDM | _abi.FAM_NGLDM
LTEX_CELLS = 8192                       # kLtexCells (roi_kernel.h): plane cells per strip workgroup, whole rows
KINDS = ("columns", "strip_runs", "shifted_runs", "diag45", "diag135", "seam_holes", "serpentine", "checker", "noise", "constant")


def seam_roi(w, h, r, kind, rng, hi=4096):
    """A w x h box (r rows per strip) whose content aims at the strip seams."""
    yy, xx = np.mgrid[0:h, 0:w]
    keep = np.ones((h, w), bool)
    lv = lambda k: 1 + (np.asarray(k) * 7919) % (hi - 1)         # distinct levels spread over the range
    if kind == "columns":                                         # constant along columns: every vertical run crosses every seam
        v = lv(xx // 3)
    elif kind == "strip_runs":                                    # vertical runs exactly one strip long, ending on the seams
        v = lv(xx + 5 * (yy // r))
    elif kind == "shifted_runs":                                  # ... one strip long, straddling the seams
        v = lv(xx + 5 * ((yy + r // 2) // r))
    elif kind == "diag45":                                        # bands that cross seams at the box edges
        v = lv((xx + yy) // 4)
    elif kind == "diag135":
        v = lv((xx - yy + h) // 4)
    elif kind == "seam_holes":                                    # noise, with holes on the rows either side of every seam
        v = rng.integers(1, hi, (h, w))
        seam = ((yy % r) == 0) | ((yy % r) == r - 1)
        keep &= ~(seam & (rng.random((h, w)) < 0.3))
    elif kind == "serpentine":                                    # one zone of level A snaking through every strip in a field of B
        v = np.full((h, w), hi // 3)
        # bands on rows 1, 5, 9, ... joined by one-pixel connectors at alternate ends (rows 2-4 at the right edge, 6-8 at the left)
        path = ((yy % 4) == 1) | ((yy >= 2) & (xx == np.where(((yy - 2) // 4) % 2 == 0, w - 1, 0)))
        v[path] = hi - 1
    elif kind == "checker":
        v = np.where((xx + yy) % 2 == 0, hi // 4, (3 * hi) // 4)
    elif kind == "noise":
        v = rng.integers(1, hi, (h, w))
    else:                                                         # constant
        v = np.full((h, w), hi // 2)
    keep[0, 0] = keep[h - 1, w - 1] = True                        # the box keeps its size
    y, x = np.nonzero(keep)
    o = np.lexsort((y, x))
    return dict(x=x[o], y=y[o], inten=np.asarray(v)[y[o], x[o]].astype(np.uint32))


def width_for(rows):
    """A box width w with kLtexCells // w == rows."""
    w = {1: 4100, 2: 2800, 3: 2100}.get(rows, LTEX_CELLS // rows)
    assert LTEX_CELLS // w == rows, (rows, w)
    return w


def check_counts(ctx, rois, mask, s, ltex=True, against_ref=True):
    """HIP against the oracle (and the reference classes when built): compare_tables, compare_counts, compare_tight.  ltex: True
    -- the strip path served the class (cooperative bit 1), False -- it did not, None -- no assertion."""
    b = _abi.batch_from_rois(rois)
    G = ctx.featurize_host(b, mask, s)
    rep = ctx.launch_report()
    names = _lib.column_names(mask, s)
    O = po.oracle_featurize(b, mask, s)
    bad = parity.compare_tables(G, O, names, batch=b) + counts.compare_counts(G, O, names) + counts.compare_tight(G, O, names)
    assert not bad, "vs oracle:\n" + "\n".join(bad[:20])
    if against_ref and po.have_ref():
        R = po.ref_featurize(b, mask, s, n_threads=4)
        bad = counts.compare_counts(G, R, names) + counts.compare_tight(G, R, names)
        assert not bad, "vs reference classes:\n" + "\n".join(bad[:20])
    if ltex is not None:
        assert any(r["cooperative"] & 2 for r in rep) == ltex, rep
    return G, rep


@pytest.mark.parametrize("rows", [1, 2, 3, 63, 64, 65])
def test_strip_seams(hip_ctx, rows):
    """Every content kind on boxes of k strips and k strips +- 1 row (k = 4, so the last strip is full, one row short or one row
    over), grey depths 8 and 64."""
    rng = np.random.default_rng(rows)
    w = width_for(rows)
    rois = [seam_roi(w, h, rows, kind, rng) for h in (4 * rows - 1, 4 * rows, 4 * rows + 1) if h >= 2 for kind in KINDS]
    for gd in (8, 64):
        check_counts(hip_ctx, rois, TEX, _abi.default_settings(gd))


@pytest.mark.parametrize("gd,ibsi", [(8, 0), (64, 0), (-16, 0), (4094, 0), (0, 1)])
def test_seam_rois_under_every_binning(hip_ctx, gd, ibsi):
    """Grey depths 8 / 64, radiomics binning (-16), the documented limit 4094, and IBSI with 1000 levels (16-bit plane)."""
    rng = np.random.default_rng(100 + gd)
    hi = 1001 if ibsi else 4096
    s = _abi.default_settings(gd if not ibsi else 8, bool(ibsi))
    rois = [seam_roi(width_for(r), 3 * r + 1, r, kind, rng, hi=hi) for r in (2, 63) for kind in ("strip_runs", "diag135", "seam_holes", "serpentine", "noise")]
    if gd != 4094:                                                 # (the oracle's GLSZM matrix is levels x box cells)
        rois.append(ellipse_roi(150, 120, rng, hi=hi))             # 56 k pixels
    check_counts(hip_ctx, rois, TEX, s)


@pytest.mark.parametrize("w,h", [(100, 100), (127, 127), (63, 300), (65, 200), (127, 300), (129, 129), (129, 257)])
def test_boxes_where_the_launch_changes_form(hip_ctx, w, h):
    """Size class 2 (up to 128 x 128 and 16384 pixels: the strip path on a lane of its own), and widths one short of / one past a
    wave and two waves on boxes of size classes 3 and 4."""
    rng = np.random.default_rng(w * h)
    rows = max(1, LTEX_CELLS // w)
    rois = [seam_roi(w, h, rows, kind, rng) for kind in ("columns", "shifted_runs", "diag45", "seam_holes", "serpentine", "checker")]
    check_counts(hip_ctx, rois, TEX, _abi.default_settings(8))


def test_one_workgroup_workspace_path(hip_ctx):
    """A box wider than the strip kernels stage (9000 x 20) goes to the one-workgroup kernel of roi_texture.hip: counts exact there
    too."""
    rng = np.random.default_rng(41)
    rois = [seam_roi(9000, 20, 1, kind, rng) for kind in ("columns", "diag45", "noise")]
    check_counts(hip_ctx, rois, TEX, _abi.default_settings(8), ltex=False, against_ref=False)
    check_counts(hip_ctx, rois, TEX, _abi.default_settings(64), ltex=False, against_ref=False)


@pytest.mark.parametrize("gd", [8, 64])
def test_dependence_trio_on_big_boxes(hip_ctx, gd):
    """GLDZM / GLDM / NGLDM (roi_dependence.hip) on 20 k .. 110 k-pixel ellipses, holes, and seam-shaped boxes."""
    rng = np.random.default_rng(gd)
    rois = [ellipse_roi(90, 72, rng), ellipse_roi(210, 166, rng, lo=0, holes=0.02), ellipse_roi(150, 120, rng, hi=300)]
    rois += [seam_roi(130, 190, 63, kind, rng) for kind in ("columns", "serpentine", "checker", "seam_holes")]
    check_counts(hip_ctx, rois, DEP, _abi.default_settings(gd), ltex=None)
