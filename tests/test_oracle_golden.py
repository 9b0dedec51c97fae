"""CPU tests: pin the plain-C oracle (oracle/nyx_oracle.c) against
  (1) the golden vectors the reference's own tests hold for the hot path, and
  (2) the reference's own classes compiled in place (oracle/_ref), bit for bit.  Their tables are kept under
      tests/golden/reference_classes/ so that (2) holds where oracle/_ref cannot be built: with the library present a
      test runs it and also checks it against the stored table; without it, the stored table stands in for it.
      NYX_WRITE_REF_GOLDEN=1 (with oracle/_ref built) rewrites the stored tables.
"""
import os

import numpy as np
import pytest

from nyxus_amd import _abi
from oracle import pyoracle as po
from tests import fixtures, synth

REF = fixtures.reference_tests()

INT = ["COV", "COVERED_IMAGE_INTENSITY_RANGE", "ENERGY", "ENTROPY", "EXCESS_KURTOSIS", "HYPERFLATNESS",
       "HYPERSKEWNESS", "INTEGRATED_INTENSITY", "INTERQUARTILE_RANGE", "KURTOSIS", "MAX", "MEAN",
       "MEAN_ABSOLUTE_DEVIATION", "MEDIAN", "MEDIAN_ABSOLUTE_DEVIATION", "MIN", "MODE", "P01", "P10", "P25",
       "P75", "P90", "P99", "QCOD", "RANGE", "ROBUST_MEAN", "ROBUST_MEAN_ABSOLUTE_DEVIATION",
       "ROOT_MEAN_SQUARED", "SKEWNESS", "STANDARD_DEVIATION", "STANDARD_DEVIATION_BIASED", "STANDARD_ERROR",
       "VARIANCE", "VARIANCE_BIASED", "UNIFORMITY", "UNIFORMITY_PIU"]
GLCM = ["GLCM_ASM", "GLCM_ACOR", "GLCM_CLUPROM", "GLCM_CLUSHADE", "GLCM_CLUTEND", "GLCM_CONTRAST",
        "GLCM_CORRELATION", "GLCM_DIFAVE", "GLCM_DIFENTRO", "GLCM_DIFVAR", "GLCM_DIS", "GLCM_ENERGY",
        "GLCM_ENTROPY", "GLCM_HOM1", "GLCM_HOM2", "GLCM_ID", "GLCM_IDN", "GLCM_IDM", "GLCM_IDMN",
        "GLCM_INFOMEAS1", "GLCM_INFOMEAS2", "GLCM_IV", "GLCM_JAVE", "GLCM_JE", "GLCM_JMAX", "GLCM_JVAR",
        "GLCM_SUMAVERAGE", "GLCM_SUMENTROPY", "GLCM_SUMVARIANCE", "GLCM_VARIANCE"]


REF_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_classes")


def _same(A, R):
    return (A.shape == R.shape) and ((A == R) | (np.isnan(A) & np.isnan(R))).all()


def ref_golden(key, compute):
    """The reference classes' output for case `key` (dict of arrays): `compute()` when oracle/_ref is built -- equal, bit
    for bit, to the stored copy tests/golden/reference_classes/<key>.npz -- else the stored copy."""
    path = os.path.join(REF_GOLDEN, key + ".npz")
    if not po.have_ref():
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    live = compute()
    if os.environ.get("NYX_WRITE_REF_GOLDEN"):
        os.makedirs(REF_GOLDEN, exist_ok=True)
        np.savez_compressed(path, **live)
    with np.load(path) as z:
        stored = {k: z[k] for k in z.files}
    assert stored.keys() == live.keys() and all(_same(live[k], stored[k]) for k in live), f"{path} differs from oracle/_ref"
    return live


def ref_table(key, b, mask, s, n_threads):
    return ref_golden(key, lambda: {"table": po.ref_featurize(b, mask, s, n_threads=n_threads)})["table"]


def agrees_gt(val, truth, frac_tol=1000.0):
    # /root/reference/tests/test_main_nyxus.h:13-24
    return abs(val - truth) <= abs(truth / frac_tol)


def _firstorder_roi(slide=False):
    r = fixtures.roi_from_triplets(REF["pixels"]["pixelIntensityFeaturesTestData"])
    if slide:
        r["slide_min"], r["slide_max"] = 0.0, 65535.0
    return _abi.batch_from_rois([r])


def test_firstorder_matlab_goldens():
    """tests/test_2d_firstorder_matlab.h:10-39 on pixelIntensityFeaturesTestData
    (default settings: STNGS_MISSING -> 24 histogram bins, constants.h:4)."""
    s = _abi.default_settings(24)
    row = dict(zip(INT, po.oracle_featurize(_firstorder_roi(True), _abi.FAM_INTENSITY, s)[0]))
    gold = REF["goldens"]["firstorder_2d_matlab_ref_vals"]
    s20 = _abi.default_settings(20)
    row20 = dict(zip(INT, po.oracle_featurize(_firstorder_roi(), _abi.FAM_INTENSITY, s20)[0]))
    for k, v in gold.items():
        if k == "UNIFORMITY":   # matched at GREYDEPTH=20, 1 % tier (test_2d_firstorder_matlab.h:68-77)
            assert agrees_gt(row20[k], v, 100.0), (k, row20[k], v)
        else:
            assert agrees_gt(row[k], v), (k, row[k], v)


def test_firstorder_regression_goldens():
    """tests/test_2d_firstorder_regression.h:9-17 (ENTROPY pinned at GREYDEPTH=20)."""
    gold = REF["goldens"]["firstorder_2d_regression_ref_vals"]
    row = dict(zip(INT, po.oracle_featurize(_firstorder_roi(), _abi.FAM_INTENSITY, _abi.default_settings(24))[0]))
    row20 = dict(zip(INT, po.oracle_featurize(_firstorder_roi(), _abi.FAM_INTENSITY, _abi.default_settings(20))[0]))
    for k, v in gold.items():
        got = row20[k] if k == "ENTROPY" else row[k]
        assert agrees_gt(got, v), (k, got, v)


def _glcm_4slice_mean(s):
    b = fixtures.ibsi_phantom_batch(REF)
    T = po.oracle_featurize(b, _abi.FAM_GLCM, s)
    na = s.glcm_n_angles
    ang = {GLCM[k]: T[:, k * na:(k + 1) * na].sum() / 16.0 for k in range(30)}
    return ang, T


def test_glcm_regression_goldens():
    """tests/test_2d_glcm_regression.h:29-61: matlab binning, 100 levels, asymmetric,
    mean over the 4 phantom slices x 4 angles, 1 % tier (:226)."""
    s = _abi.default_settings(100)
    ang, _ = _glcm_4slice_mean(s)
    for k, v in REF["goldens"]["glcm_2d_regression_ref_vals"].items():
        assert agrees_gt(ang[k], v, 100.0), (k, ang[k], v)


def test_glcm_ibsi_goldens():
    """tests/test_2d_glcm_ibsi.h:17-49: IBSI path (identity binning, symmetric)."""
    s = _abi.default_settings(0, ibsi=True)
    s.glcm_grey_depth = 0
    ang, _ = _glcm_4slice_mean(s)
    for k, v in REF["goldens"]["glcm_2d_ibsi_ref_vals"].items():
        assert agrees_gt(ang[k], v, 100.0), (k, ang[k], v)


CONFIGS = [(8, False, 4), (64, False, 4), (-16, False, 4), (100, False, 2), (20, True, 4)]


@pytest.mark.parametrize("gd,ibsi,na", CONFIGS)
def test_oracle_matches_reference_classes_bit_exact(gd, ibsi, na):
    """The restatement and the reference's own PixelIntensityFeatures / GLCMFeature
    (compiled from /root/reference in place) agree bit for bit, edge cases included."""
    rois = synth.random_rois(60, seed=3, slide=True)
    if ibsi:
        rois = [dict(r, inten=(np.asarray(r["inten"]) % 7).astype(np.uint32)) for r in rois]
    b = _abi.batch_from_rois(rois)
    s = _abi.default_settings(gd, ibsi)
    s.glcm_n_angles = na
    mask = _abi.FAM_INTENSITY | _abi.FAM_GLCM
    A = po.oracle_featurize(b, mask, s)
    R = ref_table(f"intensity_glcm_gd{gd}_ibsi{int(ibsi)}_na{na}", b, mask, s, 3)
    same = (A == R) | (np.isnan(A) & np.isnan(R))
    assert same.all(), np.argwhere(~same)[:10]


def test_oracle_matches_reference_on_bench_tile():
    b = synth.tile_batch(0)
    assert b.n_roi == 196 and int(np.diff(b.px_offset.astype(np.int64)).max()) == 2821
    s = _abi.default_settings(8)
    mask = _abi.FAM_INTENSITY | _abi.FAM_GLCM
    A = po.oracle_featurize(b, mask, s)
    R = ref_table("intensity_glcm_bench_tile", b, mask, s, 4)
    assert ((A == R) | (np.isnan(A) & np.isnan(R))).all()


GLRLM = ["GLRLM_SRE", "GLRLM_LRE", "GLRLM_GLN", "GLRLM_GLNN", "GLRLM_RLN", "GLRLM_RLNN", "GLRLM_RP", "GLRLM_GLV",
         "GLRLM_RV", "GLRLM_RE", "GLRLM_LGLRE", "GLRLM_HGLRE", "GLRLM_SRLGLE", "GLRLM_SRHGLE", "GLRLM_LRLGLE",
         "GLRLM_LRHGLE"]
GLSZM = ["GLSZM_SAE", "GLSZM_LAE", "GLSZM_GLN", "GLSZM_GLNN", "GLSZM_SZN", "GLSZM_SZNN", "GLSZM_ZP", "GLSZM_GLV",
         "GLSZM_ZV", "GLSZM_ZE", "GLSZM_LGLZE", "GLSZM_HGLZE", "GLSZM_SALGLE", "GLSZM_SAHGLE", "GLSZM_LALGLE",
         "GLSZM_LAHGLE"]
NGTDM = ["NGTDM_COARSENESS", "NGTDM_CONTRAST", "NGTDM_BUSYNESS", "NGTDM_COMPLEXITY", "NGTDM_STRENGTH"]


def _phantom_mean(fam, s, names, angled):
    T = po.oracle_featurize(fixtures.ibsi_phantom_batch(REF), fam, s)
    if angled:  # mean over 4 slices x 4 angles
        return {n: T[:, k * 4:(k + 1) * 4].sum() / 16.0 for k, n in enumerate(names)}
    return {n: T[:, k].sum() / 4.0 for k, n in enumerate(names)}


@pytest.mark.parametrize("gold,gd,ibsi", [("glrlm_2d_regression_ref_vals", 100, False), ("glrlm_2d_ibsi_ref_vals", 128, True)])
def test_glrlm_goldens(gold, gd, ibsi):
    """tests/test_2d_glrlm_regression.h:17-34 (matlab binning; the test sets GLRLMFeature::n_levels = 100, :61) and
    tests/test_2d_glrlm_ibsi.h (IBSI path): 4 phantom slices x 4 angles averaged, 1 % tier."""
    got = _phantom_mean(_abi.FAM_GLRLM, _abi.default_settings(gd, ibsi), GLRLM, True)
    for k, v in REF["goldens"][gold].items():
        assert agrees_gt(got[k], v, 100.0), (gold, k, got[k], v)


@pytest.mark.parametrize("gold,gd,ibsi", [("glszm_2d_regression_ref_vals", 64, False), ("glszm_2d_ibsi_ref_vals", 128, True)])
def test_glszm_goldens(gold, gd, ibsi):
    """tests/test_2d_glszm_regression.h:16-33 (GREYDEPTH 64, matlab) and test_2d_glszm_ibsi.h."""
    got = _phantom_mean(_abi.FAM_GLSZM, _abi.default_settings(gd, ibsi), GLSZM, False)
    for k, v in REF["goldens"][gold].items():
        assert agrees_gt(got[k], v, 100.0), (gold, k, got[k], v)


@pytest.mark.parametrize("gold,gd,ibsi", [("ngtdm_2d_regression_ref_vals", 100, False), ("ngtdm_2d_ibsi_ref_vals", 128, True)])
def test_ngtdm_goldens(gold, gd, ibsi):
    """tests/test_2d_ngtdm_regression.h:16-22 (NGTDMFeature::n_levels = 100, :40) and test_2d_ngtdm_ibsi.h."""
    got = _phantom_mean(_abi.FAM_NGTDM, _abi.default_settings(gd, ibsi), NGTDM, False)
    for k, v in REF["goldens"][gold].items():
        assert agrees_gt(got[k], v, 100.0), (gold, k, got[k], v)


GLDM = ["GLDM_SDE", "GLDM_LDE", "GLDM_GLN", "GLDM_DN", "GLDM_DNN", "GLDM_GLV", "GLDM_DV", "GLDM_DE", "GLDM_LGLE", "GLDM_HGLE",
        "GLDM_SDLGLE", "GLDM_SDHGLE", "GLDM_LDLGLE", "GLDM_LDHGLE"]
NGLDM = ["NGLDM_LDE", "NGLDM_HDE", "NGLDM_LGLCE", "NGLDM_HGLCE", "NGLDM_LDLGLE", "NGLDM_LDHGLE", "NGLDM_HDLGLE", "NGLDM_HDHGLE",
         "NGLDM_GLNU", "NGLDM_GLNUN", "NGLDM_DCNU", "NGLDM_DCNUN", "NGLDM_DCP", "NGLDM_GLM", "NGLDM_GLV", "NGLDM_DCM", "NGLDM_DCV",
         "NGLDM_DCENT", "NGLDM_DCENE"]
GLDZM = ["GLDZM_SDE", "GLDZM_LDE", "GLDZM_LGLZE", "GLDZM_HGLZE", "GLDZM_SDLGLE", "GLDZM_SDHGLE", "GLDZM_LDLGLE", "GLDZM_LDHGLE",
         "GLDZM_GLNU", "GLDZM_GLNUN", "GLDZM_ZDNU", "GLDZM_ZDNUN", "GLDZM_ZP", "GLDZM_GLM", "GLDZM_GLV", "GLDZM_ZDM", "GLDZM_ZDV",
         "GLDZM_ZDE"]


def test_gldm_goldens():
    """tests/test_2d_gldm_ibsi.h:15-119 (4 phantom slices averaged, IBSI mode, 1 % tier) and
    tests/test_2d_gldm_regression.h:22-78 (cat2500 fixture, GREYDEPTH 128 matlab binning, 0.1 % tier)."""
    got = _phantom_mean(_abi.FAM_GLDM, _abi.default_settings(128, True), GLDM, False)
    for k, v in REF["goldens"]["gldm_2d_ibsi_ref_vals"].items():
        assert agrees_gt(got[k], v, 100.0), (k, got[k], v)
    b = _abi.batch_from_rois([fixtures.roi_from_triplets(REF["pixels"]["cat2500_int"], REF["pixels"]["cat2500_seg"])])
    T = po.oracle_featurize(b, _abi.FAM_GLDM, _abi.default_settings(128, False))[0]
    for k, v in REF["goldens"]["gldm_2d_regression_ref_vals"].items():
        assert agrees_gt(T[GLDM.index(k)], v), (k, T[GLDM.index(k)], v)


@pytest.mark.parametrize("gold,tol", [("ngldm_2d_ibsi_ref_vals", 100.0), ("ngldm_2d_mirp_ref_vals", 1e9), ("ngldm_2d_regression_ref_vals", 1e9)])
def test_ngldm_goldens(gold, tol):
    """tests/test_2d_ngldm_common.h:28-139 (4 phantom slices averaged, GREYDEPTH 128, IBSI mode) against the IBSI table
    (test_2d_ngldm_ibsi.h:16-35, 1 %), the mirp 2.6.0 run (test_2d_ngldm_mirp.h:26-45, 1e-9) and Nyxus' own
    GLM / DCM pins (test_2d_ngldm_regression.h:14-18, 1e-9)."""
    got = _phantom_mean(_abi.FAM_NGLDM, _abi.default_settings(128, True), NGLDM, False)
    for k, v in REF["goldens"][gold].items():
        assert agrees_gt(got[k], v, tol), (gold, k, got[k], v)


def test_gldzm_ibsi_goldens():
    """tests/test_2d_gldzm_ibsi.h:14-183: 4 phantom slices averaged, IBSI mode; the reference's own band is 50 %
    (agrees_gt(..., 2.)), the restatement sits inside it because it is bit-identical to the class (next test)."""
    got = _phantom_mean(_abi.FAM_GLDZM, _abi.default_settings(128, True), GLDZM, False)
    for k, v in REF["goldens"]["gldzm_2d_ibsi_ref_vals"].items():
        assert agrees_gt(got[k], v, 2.0), (k, got[k], v)


@pytest.mark.parametrize("gd,ibsi", [(8, False), (64, False), (-16, False), (20, True)])
def test_dependence_families_match_reference_classes_bit_exact(gd, ibsi):
    rois = synth.random_rois(50, seed=9)
    if ibsi:
        rois = [dict(r, inten=(np.asarray(r["inten"]) % 7).astype(np.uint32)) for r in rois]
        rois = [r for r in rois if np.asarray(r["inten"]).max() > 0]
    b = _abi.batch_from_rois(rois)
    s = _abi.default_settings(gd, ibsi)
    # radiomics binning (gd < 0) makes the reference's GLDZM index one row past its matrix for level-0 zones
    # (gldzm.cpp:44-50 with :103-106): undefined behaviour, left out of the comparison
    mask = _abi.FAM_GLDM | _abi.FAM_NGLDM | (_abi.FAM_GLDZM if gd > 0 or ibsi else 0)
    A = po.oracle_featurize(b, mask, s)
    R = ref_table(f"dependence_gd{gd}_ibsi{int(ibsi)}", b, mask, s, 2)
    same = (A == R) | (np.isnan(A) & np.isnan(R))
    assert same.all(), np.argwhere(~same)[:10]


@pytest.mark.parametrize("gd,ibsi", [(8, False), (64, False), (-16, False), (20, True)])
def test_texture_families_match_reference_classes_bit_exact(gd, ibsi):
    rois = synth.random_rois(50, seed=9)
    if ibsi:  # the reference dereferences an empty set for an all-zero ROI in IBSI NGTDM (ngtdm.cpp:58)
        rois = [dict(r, inten=(np.asarray(r["inten"]) % 7).astype(np.uint32)) for r in rois]
        rois = [r for r in rois if np.asarray(r["inten"]).max() > 0]
    b = _abi.batch_from_rois(rois)
    s = _abi.default_settings(gd, ibsi)
    mask = _abi.FAM_GLRLM | _abi.FAM_GLSZM | _abi.FAM_NGTDM
    A = po.oracle_featurize(b, mask, s)
    R = ref_table(f"texture_gd{gd}_ibsi{int(ibsi)}", b, mask, s, 2)
    same = (A == R) | (np.isnan(A) & np.isnan(R))
    assert same.all(), np.argwhere(~same)[:10]


def test_gabor_truth_goldens():
    """tests/test_gabor_truth.h:27-47: 4 DSB2018 ROIs x 4 default filters, vetted vs scikit-image;
    asserted at rel 1e-3 by the reference (test_2d_gabor_skimage.cc:17), matched exactly here."""
    b = _abi.batch_from_rois([fixtures.dsb_roi(d) for d in REF["dsb2018"]])
    G = po.oracle_featurize(b, _abi.FAM_GABOR, _abi.default_settings(64))
    T = np.array(REF["gabor_truth"])
    assert G.shape == T.shape
    assert np.all(np.abs(G - T) <= np.abs(T) / 1000.0)


def test_zernike_regression_golden():
    """tests/test_2d_zernike_regression.h:12-24 on the 8x8 shape2d fixture, abs 1e-9."""
    r = fixtures.roi_from_triplets(REF["pixels"]["shape2d_morphology_intensity"], REF["pixels"]["shape2d_morphology_mask"])
    z = po.oracle_featurize(_abi.batch_from_rois([r]), _abi.FAM_ZERNIKE, _abi.default_settings(128))[0]
    want = np.array(REF["vector_goldens"]["zernike_2d_regression_ref_vals"]["ZERNIKE2D"])
    assert np.all(np.abs(z - want) <= 1e-9)


def test_gabor_zernike_match_reference_classes_bit_exact():
    rois = synth.random_rois(40, seed=4, rmax=12) + [fixtures.dsb_roi(d) for d in REF["dsb2018"]]
    b = _abi.batch_from_rois(rois)
    s = _abi.default_settings(64)
    # an 8-filter bank like BASELINE.json configs[4]
    s.gabor_n_filters = 8
    for i in range(8):
        s.gabor_f0[i] = [4.0, 16.0, 32.0, 64.0][i % 4]
        s.gabor_theta[i] = np.pi * i / 8
    mask = _abi.FAM_GABOR | _abi.FAM_ZERNIKE
    A = po.oracle_featurize(b, mask, s)
    R = ref_table("gabor8_zernike", b, mask, s, 2)
    same = (A == R) | (np.isnan(A) & np.isnan(R))
    assert same.all(), np.argwhere(~same)[:10]


# ---- 2-D geometric moments (last item) --------------------------------------------------------------------
def _moment_close(actual, golden):
    # tests/test_2d_moments_common.h:152-168: |actual - golden| <= 1e-6 * max(1, |golden|, |actual|)
    return np.isfinite(actual) and abs(actual - golden) <= 1e-6 * max(1.0, abs(golden), abs(actual))


def _check_moment_goldens(T_shape, T_inten, lists):
    for name in lists:
        for k, v in REF["moment_goldens"][name].items():
            if k in fixtures.SMOM_NAMES:
                got = T_shape[fixtures.SMOM_NAMES.index(k)]
            else:
                got = T_inten[fixtures.IMOM_NAMES.index(k)]
            assert _moment_close(got, v), (name, k, got, v)


def test_geomoment_goldens():
    """tests/test_2d_moments_regression.h:6-118 and test_2d_moments_skimage.h:6-211 (scikit-image 0.26.0 goldens): the
    48 x 40 rectangle fixture (shape + intensity moments, weighted ones included -> contour + hill-descent distances) and
    the wedge fixture (Hu invariants)."""
    s = _abi.default_settings(256)
    b = _abi.batch_from_rois([fixtures.geomoment_rectangle_roi(), fixtures.geomoment_wedge_roi()])
    T = po.oracle_featurize(b, _abi.FAM_SMOMS | _abi.FAM_IMOMS, s)
    _check_moment_goldens(T[0, :90], T[0, 90:], ["moments_2d_regression_shape_ref_vals", "moments_2d_regression_intensity_ref_vals",
                                                  "moments_2d_skimage_shape_ref_vals", "moments_2d_skimage_intensity_ref_vals",
                                                  "moments_2d_skimage_normraw_shape_ref_vals", "moments_2d_skimage_normraw_intensity_ref_vals"])
    _check_moment_goldens(T[1, :90], T[1, 90:], ["moments_2d_skimage_wedge_hu_ref_vals"])


@pytest.mark.parametrize("seed,rmax", [(9, 25), (3, 12), (5, 40)])
def test_geomoments_match_reference_classes_bit_exact(seed, rmax):
    """Contour tracing (contour.cpp:381-619), the hill-descent distance (pixel.cpp:40-70) and all 2 x 90 moments against
    ContourFeature + Smoms2D_feature + Imoms2D_feature compiled in place, bit for bit."""
    b = _abi.batch_from_rois(synth.random_rois(40, seed=seed, rmax=rmax))
    s = _abi.default_settings(8)
    mask = _abi.FAM_SMOMS | _abi.FAM_IMOMS
    A = po.oracle_featurize(b, mask, s)
    R = ref_table(f"geomoments_seed{seed}_rmax{rmax}", b, mask, s, 2)
    same = (A == R) | (np.isnan(A) & np.isnan(R))
    assert same.all(), np.argwhere(~same)[:10]


def test_reference_tile_workflow_equals_assembly_plus_oracle():
    """oracle/ref_driver.cpp nyxref_featurize_tiles (the reference's in-memory workflow with its two label scans, bench.py's
    tile-inclusive CPU baseline) against host assembly + the C oracle: same rows, same order, same values."""
    from tests import roi_assembly
    from tests import synth
    rng = np.random.default_rng(4)
    lab = synth.disk_label_tile(size=128, pitch=32, radius=12)
    I = rng.integers(0, 4096, (2, 128, 128)).astype(np.uint32)
    M = np.stack([lab, lab * 5]).astype(np.uint32)
    s = _abi.default_settings(8)
    mask = _abi.FAM_INTENSITY | _abi.FAM_GLCM

    def workflow():
        tm = []
        t_, l_, T_ = po.ref_featurize_tiles(I, M, mask, s, n_threads=2, timing=tm)
        assert len(tm) == 2 and tm[0] > 0 and tm[1] > 0
        return {"tile": np.asarray(t_), "label": np.asarray(l_), "table": T_}
    W = ref_golden("tile_workflow", workflow)
    t, l, T = W["tile"], W["label"], W["table"]
    row = 0
    for k in range(2):
        b = roi_assembly.assemble(I[k], M[k], None, None)
        O = po.oracle_featurize(b, mask, s)
        n = len(b.roi_label)
        assert np.array_equal(l[row:row + n], b.roi_label) and np.all(t[row:row + n] == k)
        assert np.array_equal(T[row:row + n], O, equal_nan=True)
        row += n
    assert row == len(l)
