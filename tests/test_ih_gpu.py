"""The 46 IBSI intensity-histogram columns on the GPU (nyxhip_ih_batch / nyxhip_ih_tiles): the HIP rows against values recorded from the
reference's own IntensityHistogramFeatures (tests/golden/ih) -- bit for bit on ih_ref.EXACT, within parity.REL_TOL on the two entropy
columns (they go through log()) --, against tests/ih_ref.py, and against themselves across every way a row can be requested."""
import json
import os

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from tests import ih_cases, ih_ref, parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = ih_cases.golden()
EX = [ih_ref.NAMES.index(c) for c in ih_ref.EXACT]
EN = [ih_ref.NAMES.index(c) for c in ih_ref.ENTROPY]
_ROWS = {}
_REF = {}


def same(a, b):
    return a.shape == b.shape and bool(ih_ref.same(a, b).all())


def rows(ctx, name):
    """The table of a case, computed once and shared."""
    if name not in _ROWS:
        _ROWS[name] = ctx.ih_host(ih_cases.batch(name), ih_cases.settings(name))
    return _ROWS[name]


def restated(name):
    if name not in _REF:
        _REF[name] = ih_ref.table(ih_cases.batch(name), ih_cases.settings(name))
    return _REF[name]


def check(got, want, tag):
    assert got.shape == want.shape
    ok = ih_ref.same(got[:, EX], want[:, EX])
    assert ok.all(), (tag, [(r, ih_ref.EXACT[c], got[r, EX[c]], want[r, EX[c]]) for r, c in np.argwhere(~ok)[:8]])
    a, w = got[:, EN], want[:, EN]
    rel = np.where(ih_ref.same(a, w), 0.0, np.abs(a - w) / np.maximum(np.abs(w), 1e-300))
    print(f"{tag}: {len(got)} ROIs; largest relative difference on the entropy columns {rel.max() if rel.size else 0.0:.3e}")
    assert (rel <= parity.REL_TOL).all(), (tag, rel.max())


@pytest.mark.parametrize("name", list(ih_cases.CASES))
def test_hip_rows_match_the_reference_class(hip_ctx, name):
    check(rows(hip_ctx, name), GOLD[name]["table"], name)


@pytest.mark.parametrize("name", list(ih_cases.CASES))
def test_hip_rows_match_the_restatement(hip_ctx, name):
    check(rows(hip_ctx, name), restated(name), name)


def test_index_and_gradient_columns_stand_in_for_the_bin_counts(hip_ctx):
    """The counts are not output: the 1-based index columns and the gradient columns, which are functions of the counts alone, are exact
    -- and they are what the recorded counts give."""
    cols = [ih_ref.NAMES.index(c) for c in ("IH_MEDIAN_IDX", "IH_MINIMUM_IDX", "IH_P10_IDX", "IH_P90_IDX", "IH_MAXIMUM_IDX", "IH_MODE_IDX",
                                            "IH_MAX_GRADIENT", "IH_MAX_GRADIENT_IDX", "IH_MIN_GRADIENT", "IH_MIN_GRADIENT_IDX", "IH_NUM_BINS")]
    g, gi, mo = ih_ref.NAMES.index("IH_MIN_GRADIENT"), ih_ref.NAMES.index("IH_MIN_GRADIENT_IDX"), ih_ref.NAMES.index("IH_MODE_IDX")
    for name in ("ramp_n2", "ramp_n3", "ramp_n64", "ramp_n4096", "sizes", "flat_big", "disks", "no_gradient"):
        got = rows(hip_ctx, name)
        assert same(got[:, cols], GOLD[name]["table"][:, cols]), name
        for r, c in enumerate(GOLD[name]["counts"]):
            c = c.astype(np.int64)
            n = len(c)
            grad = np.array([c[1] - c[0]] + [(c[i + 1] - c[i - 1]) / 2.0 for i in range(1, n - 1)] + [c[n - 1] - c[n - 2]], float)
            assert got[r, g] == grad.min() and got[r, gi] == int(np.argmin(grad)) + 1, (name, r)
            assert got[r, mo] == int(np.argmax(c)) + 1, (name, r)
    assert GOLD["flat_big"]["counts"][0].max() > 65535
    ng = rows(hip_ctx, "no_gradient")
    k = ih_ref.NAMES.index("IH_MAX_GRADIENT")
    assert (ng[:2, k] == ih_ref.DBL_MIN).all() and (ng[:2, k + 1] == 0).all() and ng[2, k] == 1.0 and ng[2, k + 1] == 1.0


def test_gate_rows_are_soft_nan(hip_ctx):
    for name in ("gates", "gate_negative_depth", "gate_ibsi_off"):
        assert (rows(hip_ctx, name) == ih_cases.SOFT_NAN).all(), name
    m = rows(hip_ctx, "mixed")
    k = ih_cases.mixed_row("gates")
    assert (m[k:k + 3] == ih_cases.SOFT_NAN).all() and not (m[k + 3] == ih_cases.SOFT_NAN).any()
    assert same(rows(hip_ctx, "five_softnan"), rows(hip_ctx, "five"))        # nothing of an ordinary row is the sentinel


def test_a_row_has_the_same_bits_however_it_is_asked_for(hip_ctx):
    import torch
    mixed = rows(hip_ctx, "mixed")
    for name in ih_cases.MIXED_AT_64:                                        # alone | in the mixed batch
        k, n = ih_cases.mixed_row(name), ih_cases.batch(name).n_roi
        assert same(rows(hip_ctx, name), mixed[k:k + n]), name
    s = ih_cases.settings("sizes")
    rois = ih_cases.CASES["sizes"]["rois"]()
    for r in range(len(rois)):                                               # each ROI alone: 63 .. 257 px, both launch forms
        assert same(hip_ctx.ih_host(_abi.batch_from_rois(rois[r:r + 1]), s), rows(hip_ctx, "sizes")[r:r + 1]), r
    assert same(hip_ctx.ih_host(ih_cases.batch("mixed"), ih_cases.settings("mixed")), mixed)      # repeatable across calls
    assert same(hip_ctx.ih_host(ih_cases.batch("ramp_n4096"), ih_cases.settings("ramp_n4096")), rows(hip_ctx, "ramp_n4096"))
    # a device batch: with the stated largest ROI and without it
    b = ih_cases.batch("mixed")
    dev = torch.device("cuda", 0)
    keep = {k: torch.from_numpy(getattr(b, k).view({4: np.int32, 8: np.int64}[getattr(b, k).dtype.itemsize])).to(dev)
            for k in ("px_offset", "inten", "min_inten", "max_inten")}
    for stated in (True, False):
        cb = _abi.Batch()
        cb.n_roi = b.n_roi
        for k, t in keep.items():
            setattr(cb, k, t.data_ptr())
        cb.memory = _abi.MEM_DEVICE
        cb.max_px = int(np.diff(b.px_offset.astype(np.int64)).max()) if stated else 0
        out = torch.full((b.n_roi, 50), -1.0, dtype=torch.float64, device=dev)
        hip_ctx.ih_device(cb, ih_cases.settings("mixed"), out.data_ptr(), 50)
        G = out.cpu().numpy()
        assert same(G[:, :46], mixed) and (G[:, 46:] == -1.0).all(), stated


def test_tile_entry(hip_ctx):
    it, lab = ih_cases.api_tile()
    b = ih_cases.tile_batch()
    s = ih_cases.settings("sizes")
    s.grey_depth = ih_cases.API_DEPTH
    want = hip_ctx.ih_host(b, s)
    check(want, GOLD["tile"]["table"], "tile")
    tiles, labels, T = hip_ctx.ih_tiles_host(it[None], lab[None], s)
    assert list(labels) == list(b.roi_label) and list(tiles) == [0] * b.n_roi and same(T, want)
    tiles, labels, T = hip_ctx.ih_tiles_host(np.stack([it] * 3), np.stack([lab] * 3), s, max_device_bytes=1 << 20)
    assert list(tiles) == [0] * b.n_roi + [1] * b.n_roi + [2] * b.n_roi and same(T, np.tile(want, (3, 1)))


def test_bin_count_cap(hip_ctx):
    b = ih_cases.batch("sizes")
    s = ih_cases.settings("sizes")
    s.grey_depth = ih_cases.N_CAP
    got = hip_ctx.ih_host(b, s)
    check(got, ih_ref.table(b, s), "N at the cap")
    s.grey_depth = ih_cases.N_CAP + 1
    with pytest.raises(_lib.NyxHipError, match="4096") as ei:
        hip_ctx.ih_host(b, s)
    assert ei.value.code == 4
    it, lab = ih_cases.api_tile()
    with pytest.raises(_lib.NyxHipError, match="4096") as ei:
        hip_ctx.ih_tiles_host(it[None], lab[None], s)
    assert ei.value.code == 4
    s.ibsi = 0                                                               # the class gates itself first
    assert (hip_ctx.ih_host(b, s) == s.soft_nan).all()


def test_through_nyxus_featurize():
    api = json.load(open(os.path.join(ROOT, "tests", "golden", "ih", "api_expected.json")))
    it, lab = ih_cases.api_tile()
    assert str(it.dtype) == api["inten_dtype"]
    en = set(ih_ref.ENTROPY)
    for case in api["cases"].values():
        nyx = nyxus_amd.Nyxus(case["features"], ibsi=True, coarse_gray_depth=api["coarse_gray_depth"])
        df = nyx.featurize(it, lab)
        assert list(df.columns[4:]) == case["columns"]
        assert list(df["ROI_label"]) == api["labels"]
        got = df[case["columns"]].values.astype(float)
        want = np.array(case["numeric"])
        assert np.isfinite(got).all()
        for c, col in enumerate(case["columns"]):
            if col in en:
                assert (np.abs(got[:, c] - want[:, c]) <= parity.REL_TOL * np.abs(want[:, c])).all(), col
            else:
                assert (got[:, c] == want[:, c]).all(), col
    # ibsi off at call time: the codes are dropped; nothing left is an error
    nyx = nyxus_amd.Nyxus(["*ALL_IH*", "MEAN"])
    assert list(nyx.featurize(it, lab).columns[4:]) == ["MEAN"]
    with pytest.raises(ValueError, match="no features requested"):
        nyxus_amd.Nyxus(["*ALL_IH*"]).featurize(it, lab)


def test_intensity_columns_do_not_move_beside_the_histogram_family():
    it, lab = ih_cases.api_tile()
    plain = nyxus_amd.Nyxus(["*ALL_INTENSITY*"], ibsi=True, coarse_gray_depth=ih_cases.API_DEPTH).featurize(it, lab)
    both = nyxus_amd.Nyxus(["*ALL_IH*", "*ALL_INTENSITY*"], ibsi=True, coarse_gray_depth=ih_cases.API_DEPTH).featurize(it, lab)
    n = len(plain.columns)
    assert list(both.columns[:n]) == list(plain.columns) and list(both.columns[n:]) == ih_ref.NAMES
    assert same(both[list(plain.columns[4:])].values.astype(float), plain[list(plain.columns[4:])].values.astype(float))
    alone = nyxus_amd.Nyxus(["*ALL_IH*"], ibsi=True, coarse_gray_depth=ih_cases.API_DEPTH).featurize(it, lab)
    assert same(both[ih_ref.NAMES].values.astype(float), alone[ih_ref.NAMES].values.astype(float))
