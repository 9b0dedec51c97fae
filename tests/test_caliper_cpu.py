"""Feret, Martin and Nassenstein diameters (NYXHIP_FAM_FERET / _MARTIN / _NASSENSTEIN), the parts that need no GPU: the column
catalogue, the feature-set plumbing, the ROI origin on the batch object, and tests/caliper_ref.py against values recorded from the
reference's own classes (tests/golden/caliper)."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib, featureset
from tests import caliper_cases, caliper_ref, outline_cases, parity

FE, MA, NA = _abi.FAM_FERET, _abi.FAM_MARTIN, _abi.FAM_NASSENSTEIN
CAL = FE | MA | NA
OUTLINE = _abi.FAM_FRACTAL | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS
GOLD = caliper_cases.golden()


def mismatches(got, want, rel=parity.REL_TOL):
    """Rows / columns of two (n, 20) tables beyond the bounds of the caliper tests: the two angles and the three modes exactly,
    every other column within `rel`."""
    bad = []
    for c, name in enumerate(caliper_ref.NAMES):
        g, w = got[:, c], want[:, c]
        ok = (g == w) if name in caliper_ref.EXACT else (np.abs(g - w) <= rel * np.abs(w))
        bad += [f"row {r} {name}: got {g[r]!r}, want {w[r]!r}" for r in np.nonzero(~ok)[0]]
    return bad


def test_bits_and_column_counts():
    assert (FE, MA, NA) == (1 << 18, 1 << 19, 1 << 20)
    assert _abi.FAM_ALL == 0xFFF and _abi.FAM_NORTH_STAR == 0x7F and not (_abi.FAM_ALL & CAL)
    lib = _lib.load()
    assert lib.nyxhip_abi_version() == 2
    assert hasattr(lib, "nyxhip_featurize_batch_at") and hasattr(lib, "nyxhip_featurize_batch_async_at")
    s = _abi.default_settings(64)
    assert [len(_lib.column_names(m, s)) for m in (FE, MA, NA, CAL)] == [8, 6, 6, 20]
    assert _lib.column_names(CAL, s) == caliper_ref.NAMES


def test_columns_sit_between_fract_dim_perimeter_and_euler_number():
    s = _abi.default_settings(64)
    names = _lib.column_names(_abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE | CAL, s)
    i = names.index
    assert i("FRACT_DIM_PERIMETER") + 1 == i("MIN_FERET_ANGLE") and i("STAT_NASSENSTEIN_DIAM_MODE") + 1 == i("EULER_NUMBER")
    assert names[i("MIN_FERET_ANGLE"):i("EULER_NUMBER")] == caliper_ref.NAMES
    # every mask without the bits keeps its columns; with them the other columns keep their order
    for m in (_abi.FAM_ALL, _abi.FAM_ALL | _abi.FAM_RADIAL | OUTLINE, _abi.FAM_INTENSITY | _abi.FAM_GLCM, OUTLINE, _abi.FAM_EULER):
        assert [n for n in _lib.column_names(m | CAL, s) if n not in caliper_ref.NAMES] == _lib.column_names(m, s)
    assert _lib.column_names(MA | _abi.FAM_GLCM, s)[:7] == caliper_ref.NAMES[8:14] + ["GLCM_ASM_0"]


def test_unassigned_bits_stay_out_of_the_catalogue():
    s = _abi.default_settings(64)
    for bit in (12, 14, 31):
        assert _lib.column_names(1 << bit, s) == []
        assert _lib.column_names(CAL | (1 << bit), s) == caliper_ref.NAMES


def test_expand_orders_by_the_served_list_and_the_frozen_lists_are_untouched():
    assert not set(caliper_ref.NAMES) & set(featureset.ENUM_ORDER) and not set(caliper_ref.NAMES) & set(featureset.OUTPUT_ORDER)
    assert len(featureset.OUTPUT_ORDER) == len(featureset.ENUM_ORDER) + 6
    assert len(featureset.SERVED_ORDER) == len(featureset.OUTPUT_ORDER) + 20
    assert [n for n in featureset.SERVED_ORDER if n not in caliper_ref.NAMES] == featureset.OUTPUT_ORDER
    k = featureset.SERVED_ORDER.index("FRACT_DIM_PERIMETER")
    assert featureset.SERVED_ORDER[k + 1:k + 21] == caliper_ref.NAMES and featureset.SERVED_ORDER[k + 21] == "EULER_NUMBER"
    mask, order = featureset.expand(["EULER_NUMBER", "STAT_MARTIN_DIAM_MODE", "MEAN", "GLCM_ASM", "MIN_FERET_ANGLE", "FRACT_DIM_BOXCOUNT"])
    assert mask == _abi.FAM_EULER | MA | FE | _abi.FAM_FRACTAL | _abi.FAM_INTENSITY | _abi.FAM_GLCM
    assert order == ["MEAN", "FRACT_DIM_BOXCOUNT", "MIN_FERET_ANGLE", "STAT_MARTIN_DIAM_MODE", "EULER_NUMBER", "GLCM_ASM"]
    s = _abi.default_settings(64)
    names = _lib.column_names(mask, s)
    sel = featureset.column_selector(order, names, [0, 45, 90, 135])
    assert [names[j] for j in sel][:5] == order[:5]
    assert featureset.expand(["stat_nassenstein_diam_median"]) == (NA, ["STAT_NASSENSTEIN_DIAM_MEDIAN"])
    for unserved in ("PERIMETER", "CIRCULARITY", "EDGE_MEAN_INTENSITY", "CONVEX_HULL_AREA", "AREA_PIXELS_COUNT"):
        with pytest.raises(ValueError, match="not served by the MI355X path"):
            featureset.expand([unserved])


def test_batches_keep_the_roi_origins():
    b = caliper_cases.batch("placed")
    assert b.origin_x.dtype == np.uint32 and b.origin_y.dtype == np.uint32
    assert list(b.origin_x[8:16]) == [4093] * 8 and list(b.origin_y[16:24]) == [17] * 8
    assert (b.x[:10] < 70).all()                                            # the coordinates stay relative to the box
    t = caliper_cases.batch("tile")
    rois = caliper_cases.tile_rois()
    assert [int(r["x"].min()) for r in rois] == list(t.origin_x) and [int(r["y"].min()) for r in rois] == list(t.origin_y)
    assert outline_cases.batch("small").origin_x is not None                # every batch built from ROI dicts carries them
    # origins that do not fit uint32 cannot cross the ABI: the batch says so instead of pretending (0, 0)
    r = caliper_cases.degenerate()[5]
    for far in (dict(r, x=r["x"] - 3), dict(r, y=r["y"] + 2 ** 32)):
        hb = _abi.batch_from_rois([far])
        assert hb.origin_x is None and hb.origin_unrepresentable
    assert not b.origin_unrepresentable
    assert not _abi.HostBatch(b.roi_label, b.px_offset, b.x, b.y, b.inten, b.bbox_w, b.bbox_h, b.min_inten, b.max_inten).origin_unrepresentable


@pytest.mark.parametrize("name", list(caliper_cases.CASES))
def test_restatement_matches_the_reference_classes(name):
    b = caliper_cases.batch(name)
    g = GOLD[name]
    off = b.px_offset.astype(np.int64)
    tab = caliper_ref.sincos_table()
    for r in range(b.n_roi):
        x, y = b.x[off[r]:off[r + 1]], b.y[off[r]:off[r + 1]]
        H = caliper_ref.hull(x, y)
        assert H == [tuple(p) for p in g["hull"][r].tolist()], r            # the vertex list, in the reference's order
        assert H == caliper_ref.hull_all_pixels(x, y), r                    # per-column extremes give the hull of all pixels
        F, M, N = caliper_ref.diameters(x, y, b.origin_x[r], b.origin_y[r], tab, H)
        for got, want in (([d for _, d in F], g["feret"][r]), (M, g["martin"][r]), (N, g["nassenstein"][r])):
            assert got == list(want[~np.isnan(want)]), r                    # the per-angle diameters, bit for bit
    bad = mismatches(caliper_ref.table(b), g["table"])
    assert not bad, "\n".join(bad[:10])


def test_degenerate_rows_and_soft_nan():
    b = caliper_cases.batch("degenerate")
    for sn, key in ((0.0, "degenerate"), (-7.5, "degenerate_softnan")):
        want = GOLD[key]["table"]
        got = caliper_ref.table(b, soft_nan=sn)
        assert (want[0] == sn).all() and (got[0] == sn).all()               # 1 pixel: no hull
        assert not mismatches(got, want)
    T = GOLD["degenerate"]["table"]
    assert (T[2:5, 14:] == 0).all() and (T[1, 14:] == 0).all()              # hulls of 2 vertices: Nassenstein has no diameters (six zeros)
    assert T[5, 14] > 0 and T[6, 14] >= 0                                   # the block and the L have some


def test_the_placement_changes_the_reference_values():
    P = GOLD["placed"]["table"].reshape(3, 8, 20)
    assert (P[0] != P[1]).any() and (P[0] != P[2]).any()
    # ... through the float rounding of the rotated vertices only: the hulls are the same
    H = GOLD["placed"]["hull"]
    assert all((H[s] == H[8 + s]).all() and (H[s] == H[16 + s]).all() for s in range(8))
    # the restatement without origins gives the rows of the first placement
    b = caliper_cases.batch("placed")
    z = np.zeros(b.n_roi, np.int64)
    assert (caliper_ref.table(b, origin=(z, z))[8:16] == caliper_ref.table(b)[:8]).all()


def test_wide_cases_straddle_the_lds_limit():
    b = caliper_cases.batch("wide")
    assert caliper_cases.LDS_COLS == 1024
    assert sorted(set(b.bbox_w.tolist())) == [1023, 1024, 1025, 1061]
