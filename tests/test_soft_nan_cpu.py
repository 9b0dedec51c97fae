"""CPU tests: the oracle's soft_nan branches against the reference's own classes at a soft_nan that is not 0.0.

At the default 0.0 "wrote soft_nan", "wrote a literal zero" and "left the cell alone" give one table, and every other comparison of
oracle and reference classes runs at the default.  Here SOFT_NAN = -7.5, on ROIs that are undefined somewhere for every family that
can be.  The reference's tables are recorded results (tests/golden/reference_classes/softnan_*.npz, through ref_golden of
tests/test_oracle_golden.py), so a checkout that cannot build oracle/_ref still compares against the reference's values."""
import numpy as np
import pytest

from nyxus_amd import _lib
from oracle import pyoracle as po
from tests import soft_nan_cases as sc
from tests.test_oracle_golden import ref_golden

SOFT_NAN = sc.SOFT_NAN
# column-name prefix of every family block that these inputs can leave undefined.  (Gabor writes soft_nan only for a ROI that is not
# constant yet has a baseline response equal in every pixel of its box, gabor.cpp:82-95; a constant ROI gets 0.0 at :53-57.)
BLOCKS = {"glcm": ["GLCM_"], "texture": ["GLRLM_", "GLSZM_", "NGTDM_"], "dependence": ["GLDZM_", "GLDM_", "NGLDM_"], "shape": ["ZERNIKE2D"]}


def same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def reference_tables(group, cfg, which):
    """(batch, mask, settings at SOFT_NAN, reference table at SOFT_NAN, reference table at 0.0) of one case."""
    mask, _ = sc.GROUPS[group]
    name, gd, ibsi, na, off = cfg
    b = sc._abi.batch_from_rois(sc.cases(group, ibsi, which))
    s, s0 = sc.settings(gd, ibsi, SOFT_NAN, na, off), sc.settings(gd, ibsi, 0.0, na, off)

    def compute():                                     # the soft_nan = 0 table is kept as its differences from the other one
        T, T0 = po.ref_featurize(b, mask, s, n_threads=2), po.ref_featurize(b, mask, s0, n_threads=2)
        at = np.flatnonzero(~same(T, T0))
        return {"table": T, "zero_at": at, "zero_value": T0.ravel()[at]}
    R = ref_golden(f"softnan_{group}_{name}_{which}", compute)
    T0 = R["table"].copy()
    T0.ravel()[R["zero_at"]] = R["zero_value"]
    return b, mask, s, R["table"], T0


def all_cases():
    return [pytest.param(g, c, w, id=f"{g}-{c[0]}-{w}") for g, (_, cfgs) in sc.GROUPS.items() for c in cfgs for w in ("degenerate", "random")]


@pytest.mark.parametrize("group,cfg,which", all_cases())
def test_oracle_equals_reference_classes_at_soft_nan(group, cfg, which):
    b, mask, s, R, R0 = reference_tables(group, cfg, which)
    names = _lib.column_names(mask, s)
    assert R.shape == (b.n_roi, len(names)) and R0.shape == R.shape
    # ---- teeth, from the reference's tables alone ----
    if group in BLOCKS:
        for p in BLOCKS[group]:
            if p == "NGTDM_" and cfg[2]:
                continue      # under IBSI the level list runs 0 .. max (ngtdm.cpp:56-62): "fewer than 2 levels" (:70-77) needs a blank ROI, which faults at :59
            cols = [j for j, n in enumerate(names) if n.startswith(p)]
            assert cols and (R[:, cols] == SOFT_NAN).any(), f"no {p}* cell of the reference's table holds soft_nan"
        assert not same(R, R0).all()
        if group == "glcm":
            early = (R == 0.0).all(axis=1)                               # glcm.cpp:27-95 undone by save_value (:210-215)
            assert early.any() and (R[~early] == SOFT_NAN).any()         # blank matrix :260-295, f_corr :636-639, f_info_meas_corr1 :880-883
    else:                                                                # the moment families and INTENSITY never write soft_nan
        assert not (R == SOFT_NAN).any() and same(R, R0).all()
        if group == "moments":
            assert np.isnan(R).any()                                     # what they leave undefined stays a raw NaN
    # ---- the oracle ----
    A = po.oracle_featurize(b, mask, s)
    diff = ~same(A, R)
    rows = np.nonzero(diff.any(axis=1))[0]
    assert not diff.any(), (f"{int(diff.sum())} cells in {len(rows)} rows differ; rows {rows[:12].tolist()} have min == max: "
                            f"{(b.min_inten[rows[:12]] == b.max_inten[rows[:12]]).tolist()}; first: "
                            + ", ".join(f"{names[j]} roi {i}: oracle {A[i, j]!r} reference {R[i, j]!r}" for i, j in np.argwhere(diff)[:4]))
    A0 = po.oracle_featurize(b, mask, sc.settings(cfg[1], cfg[2], 0.0, cfg[3], cfg[4]))
    assert same(A0, R0).all()
