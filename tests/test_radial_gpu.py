"""Radial intensity distribution (NYXHIP_FAM_RADIAL) on the GPU: the HIP rows against tables recorded from the reference's own
classes (tests/golden/radial), against tests/radial_ref.py on other inputs, and against themselves across every way a row can
be requested.  FRAC_AT_D and MEAN_FRAC are integer counts / sums and one IEEE division each: bit-exact.  RADIAL_CV is held to the
project's relative tolerance (parity.REL_TOL)."""
import json
import os
import subprocess

import numpy as np
import pytest

import nyxus_amd
from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import parity, radial_cases, radial_ref, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = os.path.join(ROOT, "tests", "cpp", "radial_fp64_probe.hip")
PROBE_BIN = os.path.join(ROOT, "tests", "cpp", "radial_fp64_probe.bin")
R = _abi.FAM_RADIAL


def radial_of(ctx, b, mask, s):
    """(radial columns in radial_ref.NAMES order, the other columns, their names) of one call."""
    names = _lib.column_names(mask, s)
    T = ctx.featurize_host(b, mask, s)
    idx = radial_ref.split_columns(names)
    rest = [i for i in range(len(names)) if i not in set(idx)]
    return T[:, idx], T[:, rest], [names[i] for i in rest]


def test_fp64_sqrt_and_division_are_correctly_rounded(tmp_path):
    """The ring of a pixel is int(sqrt(d2) / sqrt(c2) * 7) in fp64.  IEEE sqrt and division are correctly rounded, so the device
    must return numpy's bits: integer arguments, perfect squares, and the k^2 / (49 m^2) pairs whose quotient times 7 is an
    integer -- the ring boundaries."""
    if not os.path.exists(PROBE_BIN) or os.path.getmtime(PROBE_BIN) < os.path.getmtime(PROBE_SRC):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-o", PROBE_BIN, PROBE_SRC],
                       check=True, capture_output=True, text=True)
    rng = np.random.default_rng(1)
    a = np.arange(0, 4097, dtype=np.uint64)
    c = np.concatenate([np.arange(1, 65), 49 * np.arange(1, 21) ** 2, rng.integers(1, 2 ** 31, 40)]).astype(np.uint64)
    A, Cc = np.meshgrid(a, c, indexing="ij")
    k = np.arange(0, 2000, dtype=np.uint64)
    m = np.arange(1, 60, dtype=np.uint64)
    Kk, Mm = np.meshgrid(k, m, indexing="ij")
    big = rng.integers(0, 2 ** 33, (200000, 2)).astype(np.uint64)
    big[:, 1] += 1
    pairs = np.concatenate([np.stack([A.ravel(), Cc.ravel()], 1), np.stack([(Kk * Kk).ravel(), (49 * Mm * Mm).ravel()], 1), big])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        fh.write(np.uint64(len(pairs)).tobytes())
        fh.write(np.ascontiguousarray(pairs).tobytes())
    r = subprocess.run([PROBE_BIN, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(fout, np.float64).reshape(-1, 4)
    sa, sc = np.sqrt(pairs[:, 0].astype(np.float64)), np.sqrt(pairs[:, 1].astype(np.float64))
    rat = sa / sc
    t = rat * 7.0
    ring = np.minimum(t.astype(np.int64), 7)
    print(f"fp64 probe: {len(pairs)} pairs")
    assert (got[:, 0] == sa).all() and (got[:, 1] == rat).all() and (got[:, 2] == t).all() and (got[:, 3] == ring).all()


@pytest.mark.parametrize("name", list(radial_cases.CASES))
def test_hip_rows_match_the_reference_classes(hip_ctx, name):
    b = radial_cases.batch(name)
    want = radial_cases.golden()[name]["table"]
    s = _abi.default_settings(64)
    got = hip_ctx.featurize_host(b, R, s)
    assert _lib.column_names(R, s) == radial_ref.NAMES
    bad = parity.compare_tables(got, want, radial_ref.NAMES, exact=radial_ref.EXACT)
    cv_same = (got[:, 16:] == want[:, 16:])
    print(f"{name}: {b.n_roi} ROIs; RADIAL_CV bit-identical in {int(cv_same.sum())} of {cv_same.size} values")
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("name", ["rand_seed9_rmax25", "special", "heavy"])
def test_rows_do_not_depend_on_the_companions(hip_ctx, name):
    """Alone / with the moments (the shared contour) / with every other family: the same bits; the other columns against the
    oracle, called with the mask minus the new bit."""
    b = radial_cases.batch(name)
    s = _abi.default_settings(64)
    alone, _, _ = radial_of(hip_ctx, b, R, s)
    for extra in (_abi.FAM_SMOMS | _abi.FAM_IMOMS, _abi.FAM_SMOMS, _abi.FAM_GABOR | _abi.FAM_ZERNIKE, _abi.FAM_ALL):
        got, rest, rest_names = radial_of(hip_ctx, b, R | extra, s)
        assert (got == alone).all(), (name, extra, np.argwhere(got != alone)[:5])
        assert rest_names == _lib.column_names(extra, s)
        want = po.oracle_featurize(b, extra, s)
        bad = parity.compare_tables(rest, want, rest_names, batch=b)
        assert not bad, (extra, bad[:10])
        # ... and those columns are what the call without the new bit returns
        plain = hip_ctx.featurize_host(b, extra, s)
        assert ((plain == rest) | (np.isnan(plain) & np.isnan(rest))).all(), extra


def test_tile_path_and_device_budget(hip_ctx):
    """The fused tile path (label scan + assembly + reduce) and a 2 MiB device budget over a stack of tiles return the rows of
    the batch path, bit for bit."""
    it, lab = radial_cases.tile()
    b = radial_cases.batch("tile")
    s = _abi.default_settings(64)
    want = radial_cases.golden()["tile"]["table"]
    alone = hip_ctx.featurize_host(b, R, s)
    labels, T = hip_ctx.featurize_tile_host(it, lab, R, s)
    assert list(labels) == list(b.roi_label) and (T == alone).all()
    assert not parity.compare_tables(T, want, radial_ref.NAMES, exact=radial_ref.EXACT)
    mask = R | _abi.FAM_INTENSITY | _abi.FAM_SMOMS
    names = _lib.column_names(mask, s)
    I, M = np.stack([it] * 5), np.stack([lab] * 5)
    one = hip_ctx.featurize_tiles_host(I, M, mask, s, max_device_bytes=1 << 34)
    many = hip_ctx.featurize_tiles_host(I, M, mask, s, max_device_bytes=2 << 20)
    assert (one[0] == many[0]).all() and (one[1] == many[1]).all()
    assert ((one[2] == many[2]) | (np.isnan(one[2]) & np.isnan(many[2]))).all()
    idx = radial_ref.split_columns(names)
    assert (many[2][:, idx] == np.tile(alone, (5, 1))).all()


def test_other_inputs_against_the_restatement(hip_ctx):
    """radial_ref (pinned to the reference classes by tests/test_radial_cpu.py) on inputs no fixture holds: another seed, permuted
    pixel orders (the centre's tie-break follows the caller's order), exact discs (ring and wedge boundaries are dense)."""
    rois = synth.random_rois(30, seed=77, rmax=30)
    rng = np.random.default_rng(5)
    for r in rois[:15]:
        p = rng.permutation(len(r["x"]))
        r["x"], r["y"], r["inten"] = r["x"][p], r["y"][p], r["inten"][p]
    rois += [radial_cases._mask_roi(radial_cases.disc(k), 100 + k) for k in (3, 7, 14, 21, 28)]
    b = _abi.batch_from_rois(rois)
    s = _abi.default_settings(64)
    want, D = radial_ref.radial_table(b, with_dst2=True)
    got = hip_ctx.featurize_host(b, R, s)
    defined = np.array([d != 0 for d in D])                 # (dstOC == 0 is undefined in the reference; none is expected here)
    assert defined.all()
    bad = parity.compare_tables(got, want, radial_ref.NAMES, exact=radial_ref.EXACT)
    assert not bad, "\n".join(bad[:10])


def test_through_nyxus_featurize():
    api = json.load(open(os.path.join(ROOT, "tests", "golden", "radial", "api_expected.json")))
    it, lab = radial_cases.tile()
    for case in api["cases"].values():
        nyx = nyxus_amd.Nyxus(case["features"])
        df = nyx.featurize(it.astype(api["inten_dtype"]), lab)
        assert list(df.columns[-len(case["columns"]):]) == case["columns"]
        assert list(df["ROI_label"]) == api["labels"]
        got = df[case["columns"]].values.astype(float)
        bad = parity.compare_tables(got, np.array(case["numeric"]), case["columns"], exact=radial_ref.EXACT)
        assert not bad, "\n".join(bad[:10])
    with pytest.raises(ValueError, match="not served by the MI355X path"):
        nyxus_amd.Nyxus(["PERIMETER"])


def test_unassigned_bits_are_still_bad_masks(hip_ctx):
    b = radial_cases.batch("shape2d")
    for bit in (12, 14, 31):
        with pytest.raises(_lib.NyxHipError) as ei:
            hip_ctx.featurize_host(b, R | (1 << bit), _abi.default_settings(8))
        assert ei.value.code == 1
