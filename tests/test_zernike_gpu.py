"""ZERNIKE2D on the GPU against the operation itself: every case of tests/zernike_cases.py through roi_zernike_kernel, all 30 columns
within L(npx) units of the committed exact values (tests/golden/zernike; tests/zernike_ref.py for the unit and the derived bound).  The
bound is absolute and five orders tighter than parity.REL_TOL on any moment above 1e-4: a wrong in/out decision on one disc-edge pixel, a
dropped or doubled element at the staging cap or at a stride tail, or a recombination coefficient off by one all move a row by thousands of
units.  Each test prints the worst observed |got - exact| / unit of its group (DESIGN.md section 4.4 records them)."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from tests import zernike_cases as zc
from tests import zernike_ref as zr

pytestmark = pytest.mark.gpu

GOLD = zc.golden()
ZE = _abi.FAM_ZERNIKE
THREE = _abi.FAM_GABOR | _abi.FAM_ZERNIKE | _abi.FAM_INTENSITY
_ALONE = {}


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def zernike_columns(ctx, names, mask):
    """The 30 ZERNIKE2D columns of one call over the named cases."""
    s = _abi.default_settings(64)
    T = ctx.featurize_host(zc.batch(names), mask, s)
    idx = [i for i, n in enumerate(_lib.column_names(mask, s)) if n.startswith("ZERNIKE2D_Z")]
    assert len(idx) == 30 and T.shape[0] == len(names)
    return np.ascontiguousarray(T[:, idx])


def alone(ctx, name):
    """The row of a case that runs alone, computed once."""
    if name not in _ALONE:
        _ALONE[name] = zernike_columns(ctx, [name], ZE)[0]
    return _ALONE[name]


def check(label, names, rows):
    """Every row within L(npx) units of its exact row; prints the worst ratio of the group."""
    ratios = [np.abs(row - GOLD[n]["exact"]) / zr.UNITS for n, row in zip(names, rows)]
    k = int(np.argmax([np.nanmax(np.where(np.isnan(r), np.inf, r)) for r in ratios]))
    print(f"{label}: worst |got - exact| / unit = {ratios[k].max():.2f} ({names[k]}, column {zr.PAIRS[int(ratios[k].argmax())]}, "
          f"L = {zr.bound(GOLD[names[k]]['npx'])})")
    for n, row, ratio in zip(names, rows, ratios):
        L = zr.bound(GOLD[n]["npx"])
        assert np.isfinite(row).all() and (ratio <= L).all(), (label, n, L, float(ratio.max()), zr.PAIRS[int(ratio.argmax())],
                                                               float(row[int(ratio.argmax())]), float(GOLD[n]["exact"][int(ratio.argmax())]))


@pytest.mark.parametrize("group", ["edge", "centre", "aspect", "sizes", "coeff", "aux"])
def test_every_case_alone_is_within_the_bound(hip_ctx, group):
    names = zc.GROUPS[group]
    check(group, names, [alone(hip_ctx, n) for n in names])


def test_staging_cap_in_one_launch(hip_ctx):
    """4095, 4096 and 4097 pixels beside a 5000-pixel companion of their size class: the cap is 4096, so 4096 is staged in LDS and 4097
    re-read from memory by the same launch.  Both four-wave forms read the same values in the same order: the rows are the rows of the
    clouds alone, bit for bit."""
    names = list(zc.CAP_TRIO) + ["ragged_4099", "companion_5000"]
    rows = zernike_columns(hip_ctx, names, ZE)
    check("cap batch", names, rows)
    for n, row in zip(names, rows):
        assert same(row, alone(hip_ctx, n)), n
    front = zernike_columns(hip_ctx, ["companion_5000"] + list(zc.CAP_TRIO), ZE)                     # the companion first
    assert same(front[1:], rows[:3]) and same(front[0], rows[4])


def test_three_families_move_the_columns_and_split_the_classes(hip_ctx):
    """GABOR | ZERNIKE | INTENSITY: another column offset, and the intensity family splits the batch by intensity range as well."""
    names = list(zc.CAP_TRIO) + ["companion_5000"]
    check("cap batch, three families", names, zernike_columns(hip_ctx, names, THREE))
    names = zc.GROUPS["edge"]
    check("edge batch, three families", names, zernike_columns(hip_ctx, names, THREE))
    check("edge batch", names, zernike_columns(hip_ctx, names, ZE))


def test_one_wave_and_four_wave_forms(hip_ctx):
    """A cloud of the smallest size class alone (one wave per ROI) and beside a 40 x 40 companion; a cloud of as few pixels whose box puts
    it in the next class (four waves).  Every row is within the bound; the forms add in different orders and need not agree in bits."""
    pair = zernike_columns(hip_ctx, [zc.CLASS0, "companion_40x40"], ZE)
    check("class 0 beside 40 x 40", [zc.CLASS0, "companion_40x40"], pair)
    check("class 0 alone", [zc.CLASS0], [alone(hip_ctx, zc.CLASS0)])
    small = [n for n in zc.GROUPS["sizes"] if GOLD[n]["npx"] <= 256]
    mixed = zernike_columns(hip_ctx, small + ["companion_40x40"], ZE)
    check("small clouds beside 40 x 40", small + ["companion_40x40"], mixed)
    assert same(mixed[-1], pair[1])


def test_empty_disc_is_thirty_positive_zeros(hip_ctx):
    """N = 1 and the centroid in the gap between two blobs: no pixel is inside the disc.  Zeros -- not NaN, not soft_nan."""
    s = _abi.default_settings(64)
    s.soft_nan = -7.5
    for row in (alone(hip_ctx, "empty_disc"), hip_ctx.featurize_host(zc.batch(["empty_disc"]), ZE, s)[0],
                zernike_columns(hip_ctx, ["companion_40x40", "empty_disc"], ZE)[1]):
        assert row.shape == (30,) and (row == 0.0).all() and not np.signbit(row).any(), row
