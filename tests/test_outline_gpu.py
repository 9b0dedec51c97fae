"""Fractal dimension, Euler number and ROI radius on the GPU: the HIP rows against tables recorded from the reference's own classes
(tests/golden/outline), against tests/outline_ref.py on other inputs, and against themselves across every way a row can be
requested.  EULER_NUMBER, ROI_RADIUS_MAX and ROI_RADIUS_MEDIAN are integers (or halves): bit-exact.  ROI_RADIUS_MEAN is one
division of an exact sum where the reference runs a Welford mean: parity.REL_TOL.  The two dimensions: REL_TOL relative or
outline_cases.DIM_ATOL absolute."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import outline_cases, outline_ref, parity, radial_cases, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, E, RR = _abi.FAM_FRACTAL, _abi.FAM_EULER, _abi.FAM_ROI_RADIUS
NEW = F | E | RR


def outline_of(ctx, b, mask, s):
    """(the outline columns present in `mask`, their names, the other columns, their names) of one call."""
    names = _lib.column_names(mask, s)
    T = ctx.featurize_host(b, mask, s)
    idx = [i for i, n in enumerate(names) if n in outline_cases.NAMES]
    rest = [i for i in range(len(names)) if i not in set(idx)]
    return T[:, idx], [names[i] for i in idx], T[:, rest], [names[i] for i in rest]


def same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


@pytest.mark.parametrize("name", list(outline_cases.CASES))
def test_hip_rows_match_the_reference_classes(hip_ctx, name):
    b = outline_cases.batch(name)
    want = outline_cases.golden()[name]["table"]
    s = _abi.default_settings(64)
    got = hip_ctx.featurize_host(b, NEW, s)
    assert _lib.column_names(NEW, s) == outline_cases.NAMES
    d = np.abs(got - want)
    print(f"{name}: {b.n_roi} ROIs; largest differences per column {d.max(0)}")
    bad = outline_cases.mismatches(got, want, parity.REL_TOL)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("name", ["small", "heavy"])
def test_rows_do_not_depend_on_the_companions(hip_ctx, name):
    """Alone / with each other / with the moments and the radial distribution (the shared contour) / with INTENSITY | GLCM (the moved
    column bases) / with every family: the same bits; the other columns are those of the call without the new bits, and hold
    against the oracle."""
    b = outline_cases.batch(name)
    s = _abi.default_settings(64)
    allsix = hip_ctx.featurize_host(b, NEW, s)
    col = {n: allsix[:, i] for i, n in enumerate(outline_cases.NAMES)}
    for fam in (F, E, RR, F | E, E | RR, F | RR):
        got, names, _, _ = outline_of(hip_ctx, b, fam, s)
        assert all(same(got[:, i], col[n]) for i, n in enumerate(names)), fam
    extras = [_abi.FAM_SMOMS | _abi.FAM_IMOMS | _abi.FAM_RADIAL, _abi.FAM_INTENSITY | _abi.FAM_GLCM, _abi.FAM_GLCM, _abi.FAM_INTENSITY,
              _abi.FAM_GLRLM | _abi.FAM_GLDZM | _abi.FAM_GABOR, _abi.FAM_ALL, _abi.FAM_ALL | _abi.FAM_RADIAL]
    for extra in extras:
        for fam in (NEW, E):
            got, names, rest, rest_names = outline_of(hip_ctx, b, fam | extra, s)
            assert all(same(got[:, i], col[n]) for i, n in enumerate(names)), (fam, extra)
            assert rest_names == _lib.column_names(extra, s)
            plain = hip_ctx.featurize_host(b, extra, s)
            assert same(plain, rest), (fam, extra, np.argwhere(~((plain == rest) | (np.isnan(plain) & np.isnan(rest))))[:5])
        if not extra & _abi.FAM_RADIAL:
            want = po.oracle_featurize(b, extra, s)
            bad = parity.compare_tables(rest, want, rest_names, batch=b)
            assert not bad, (extra, bad[:10])


def test_tile_path_and_device_budget(hip_ctx):
    """The fused tile path and a 2 MiB device budget over a stack of tiles return the rows of the batch path, bit for bit."""
    it, lab = radial_cases.tile()
    b = outline_cases.batch("tile")
    s = _abi.default_settings(64)
    alone = hip_ctx.featurize_host(b, NEW, s)
    labels, T = hip_ctx.featurize_tile_host(it, lab, NEW, s)
    assert list(labels) == list(b.roi_label) and same(T, alone)
    assert not outline_cases.mismatches(T, outline_cases.golden()["tile"]["table"], parity.REL_TOL)
    mask = NEW | _abi.FAM_INTENSITY | _abi.FAM_GLCM | _abi.FAM_SMOMS
    names = _lib.column_names(mask, s)
    I, M = np.stack([it] * 5), np.stack([lab] * 5)
    one = hip_ctx.featurize_tiles_host(I, M, mask, s, max_device_bytes=1 << 34)
    many = hip_ctx.featurize_tiles_host(I, M, mask, s, max_device_bytes=2 << 20)
    assert (one[0] == many[0]).all() and (one[1] == many[1]).all() and same(one[2], many[2])
    idx = outline_ref.split_columns(names)
    assert same(many[2][:, idx], np.tile(alone, (5, 1)))
    plain = hip_ctx.featurize_tiles_host(I, M, mask & ~NEW, s, max_device_bytes=2 << 20)
    rest = [i for i in range(len(names)) if i not in set(idx)]
    assert same(plain[2], many[2][:, rest])


def test_other_inputs_against_the_restatement(hip_ctx):
    """outline_ref (pinned to the reference classes by tests/test_outline_cpu.py) on inputs no fixture holds: another seed, and the
    same ROIs with permuted pixel orders -- all six columns unchanged bit for bit."""
    rois = synth.random_rois(24, seed=78, rmax=25) + [radial_cases._mask_roi(radial_cases.disc(k), 100 + k) for k in (3, 16, 17, 33)]
    b = _abi.batch_from_rois(rois)
    s = _abi.default_settings(64)
    want = outline_ref.outline_table(b)
    assert np.isfinite(want).all()
    got = hip_ctx.featurize_host(b, NEW, s)
    bad = outline_cases.mismatches(got, want, parity.REL_TOL)
    assert not bad, "\n".join(bad[:10])
    rng = np.random.default_rng(6)
    for r in rois:
        p = rng.permutation(len(r["x"]))
        r["x"], r["y"], r["inten"] = r["x"][p], r["y"][p], r["inten"][p]
    perm = hip_ctx.featurize_host(_abi.batch_from_rois(rois), NEW, s)
    assert same(perm, got), np.argwhere(perm != got)[:5]


def test_through_nyxus_featurize():
    api = json.load(open(os.path.join(ROOT, "tests", "golden", "outline", "api_expected.json")))
    it, lab = radial_cases.tile()
    for case in api["cases"].values():
        nyx = nyxus_amd.Nyxus(case["features"])
        df = nyx.featurize(it.astype(api["inten_dtype"]), lab)
        assert list(df.columns[-len(case["columns"]):]) == case["columns"]
        assert list(df["ROI_label"]) == api["labels"]
        got = df[case["columns"]].values.astype(float)
        want = np.array(case["numeric"])
        full_g, full_w = np.full((len(got), 6), np.nan), np.full((len(got), 6), np.nan)
        for j, c in enumerate(case["columns"]):
            full_g[:, outline_cases.NAMES.index(c)], full_w[:, outline_cases.NAMES.index(c)] = got[:, j], want[:, j]
        bad = outline_cases.mismatches(full_g, full_w, parity.REL_TOL)
        assert not bad, "\n".join(bad[:10])
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["PERIMETER"])


def test_unassigned_bits_are_still_bad_masks(hip_ctx):
    b = outline_cases.batch("tile")
    for bit in (12, 14, 31):
        with pytest.raises(_lib.NyxHipError) as ei:
            hip_ctx.featurize_host(b, NEW | (1 << bit), _abi.default_settings(8))
        assert ei.value.code == 1
