"""Feature names, groups and column selection for the families the HIP path covers.

Names and order mirror the reference's `Feature2D` enum
(/root/reference/src/nyx/featureset.h:12-46, 174-233, 236-268, 271-288, 291-306, 309-343, 346-357), its user-facing
names (src/nyx/featureset.cpp `UserFacingFeatureNames`) and group tokens
(`UserFacing2dFeaturegroupNames`, featureset.cpp:650-665).
"""
from __future__ import annotations

from typing import Dict, List, Tuple

from . import _abi

INTENSITY = ["COV", "COVERED_IMAGE_INTENSITY_RANGE", "ENERGY", "ENTROPY", "EXCESS_KURTOSIS", "HYPERFLATNESS",
             "HYPERSKEWNESS", "INTEGRATED_INTENSITY", "INTERQUARTILE_RANGE", "KURTOSIS", "MAX", "MEAN",
             "MEAN_ABSOLUTE_DEVIATION", "MEDIAN", "MEDIAN_ABSOLUTE_DEVIATION", "MIN", "MODE", "P01", "P10", "P25",
             "P75", "P90", "P99", "QCOD", "RANGE", "ROBUST_MEAN", "ROBUST_MEAN_ABSOLUTE_DEVIATION",
             "ROOT_MEAN_SQUARED", "SKEWNESS", "STANDARD_DEVIATION", "STANDARD_DEVIATION_BIASED", "STANDARD_ERROR",
             "VARIANCE", "VARIANCE_BIASED", "UNIFORMITY", "UNIFORMITY_PIU"]
GLCM_ANGLED = ["GLCM_ASM", "GLCM_ACOR", "GLCM_CLUPROM", "GLCM_CLUSHADE", "GLCM_CLUTEND", "GLCM_CONTRAST",
               "GLCM_CORRELATION", "GLCM_DIFAVE", "GLCM_DIFENTRO", "GLCM_DIFVAR", "GLCM_DIS", "GLCM_ENERGY",
               "GLCM_ENTROPY", "GLCM_HOM1", "GLCM_HOM2", "GLCM_ID", "GLCM_IDN", "GLCM_IDM", "GLCM_IDMN",
               "GLCM_INFOMEAS1", "GLCM_INFOMEAS2", "GLCM_IV", "GLCM_JAVE", "GLCM_JE", "GLCM_JMAX", "GLCM_JVAR",
               "GLCM_SUMAVERAGE", "GLCM_SUMENTROPY", "GLCM_SUMVARIANCE", "GLCM_VARIANCE"]
GLCM_AVE = ["GLCM_ASM_AVE", "GLCM_ACOR_AVE", "GLCM_CLUPROM_AVE", "GLCM_CLUSHADE_AVE", "GLCM_CLUTEND_AVE",
            "GLCM_CONTRAST_AVE", "GLCM_CORRELATION_AVE", "GLCM_DIFAVE_AVE", "GLCM_DIFENTRO_AVE", "GLCM_DIFVAR_AVE",
            "GLCM_DIS_AVE", "GLCM_ENERGY_AVE", "GLCM_ENTROPY_AVE", "GLCM_HOM1_AVE", "GLCM_ID_AVE", "GLCM_IDN_AVE",
            "GLCM_IDM_AVE", "GLCM_IDMN_AVE", "GLCM_IV_AVE", "GLCM_JAVE_AVE", "GLCM_JE_AVE", "GLCM_INFOMEAS1_AVE",
            "GLCM_INFOMEAS2_AVE", "GLCM_VARIANCE_AVE", "GLCM_JMAX_AVE", "GLCM_JVAR_AVE", "GLCM_SUMAVERAGE_AVE",
            "GLCM_SUMENTROPY_AVE", "GLCM_SUMVARIANCE_AVE"]
GLRLM_ANGLED = ["GLRLM_SRE", "GLRLM_LRE", "GLRLM_GLN", "GLRLM_GLNN", "GLRLM_RLN", "GLRLM_RLNN", "GLRLM_RP",
                "GLRLM_GLV", "GLRLM_RV", "GLRLM_RE", "GLRLM_LGLRE", "GLRLM_HGLRE", "GLRLM_SRLGLE", "GLRLM_SRHGLE",
                "GLRLM_LRLGLE", "GLRLM_LRHGLE"]
GLRLM_AVE = [n + "_AVE" for n in GLRLM_ANGLED]
GLSZM = ["GLSZM_SAE", "GLSZM_LAE", "GLSZM_GLN", "GLSZM_GLNN", "GLSZM_SZN", "GLSZM_SZNN", "GLSZM_ZP", "GLSZM_GLV",
         "GLSZM_ZV", "GLSZM_ZE", "GLSZM_LGLZE", "GLSZM_HGLZE", "GLSZM_SALGLE", "GLSZM_SAHGLE", "GLSZM_LALGLE",
         "GLSZM_LAHGLE"]
GLDZM = ["GLDZM_SDE", "GLDZM_LDE", "GLDZM_LGLZE", "GLDZM_HGLZE", "GLDZM_SDLGLE", "GLDZM_SDHGLE", "GLDZM_LDLGLE", "GLDZM_LDHGLE",
         "GLDZM_GLNU", "GLDZM_GLNUN", "GLDZM_ZDNU", "GLDZM_ZDNUN", "GLDZM_ZP", "GLDZM_GLM", "GLDZM_GLV", "GLDZM_ZDM", "GLDZM_ZDV",
         "GLDZM_ZDE"]
GLDM = ["GLDM_SDE", "GLDM_LDE", "GLDM_GLN", "GLDM_DN", "GLDM_DNN", "GLDM_GLV", "GLDM_DV", "GLDM_DE", "GLDM_LGLE", "GLDM_HGLE",
        "GLDM_SDLGLE", "GLDM_SDHGLE", "GLDM_LDLGLE", "GLDM_LDHGLE"]
NGLDM = ["NGLDM_LDE", "NGLDM_HDE", "NGLDM_LGLCE", "NGLDM_HGLCE", "NGLDM_LDLGLE", "NGLDM_LDHGLE", "NGLDM_HDLGLE", "NGLDM_HDHGLE",
         "NGLDM_GLNU", "NGLDM_GLNUN", "NGLDM_DCNU", "NGLDM_DCNUN", "NGLDM_DCP", "NGLDM_GLM", "NGLDM_GLV", "NGLDM_DCM", "NGLDM_DCV",
         "NGLDM_DCENT", "NGLDM_DCENE"]
NGTDM = ["NGTDM_COARSENESS", "NGTDM_CONTRAST", "NGTDM_BUSYNESS", "NGTDM_COMPLEXITY", "NGTDM_STRENGTH"]

_PQ13 = ["00", "01", "02", "03", "10", "11", "12", "13", "20", "21", "22", "23", "30"]
_PQ16 = ["%d%d" % (p, q) for p in range(4) for q in range(4)]
_PQ7 = ["02", "03", "11", "12", "20", "21", "30"]
_PQ10 = ["00", "01", "02", "03", "10", "11", "12", "20", "21", "30"]
SMOMS = (["SPAT_MOMENT_" + k for k in _PQ13] + ["CENTRAL_MOMENT_" + k for k in _PQ16] + ["NORM_SPAT_MOMENT_" + k for k in _PQ16]
         + ["NORM_CENTRAL_MOMENT_" + k for k in _PQ7] + ["HU_M%d" % k for k in range(1, 8)] + ["WEIGHTED_SPAT_MOMENT_" + k for k in _PQ10]
         + ["WEIGHTED_CENTRAL_MOMENT_" + k for k in _PQ7] + ["WT_NORM_CTR_MOM_" + k for k in _PQ7] + ["WEIGHTED_HU_M%d" % k for k in range(1, 8)])
IMOMS = (["IMOM_RM_" + k for k in _PQ13] + ["IMOM_CM_" + k for k in _PQ16] + ["IMOM_NRM_" + k for k in _PQ16] + ["IMOM_NCM_" + k for k in _PQ7]
         + ["IMOM_HU%d" % k for k in range(1, 8)] + ["IMOM_WRM_" + k for k in _PQ10] + ["IMOM_WCM_" + k for k in _PQ7]
         + ["IMOM_WNCM_" + k for k in _PQ7] + ["IMOM_WHU%d" % k for k in range(1, 8)])

# feature name -> family bit
FAMILY_OF: Dict[str, int] = {}
for _n in INTENSITY:
    FAMILY_OF[_n] = _abi.FAM_INTENSITY
for _n in GLCM_ANGLED + GLCM_AVE:
    FAMILY_OF[_n] = _abi.FAM_GLCM
for _n in GLRLM_ANGLED + GLRLM_AVE:
    FAMILY_OF[_n] = _abi.FAM_GLRLM
for _n in GLSZM:
    FAMILY_OF[_n] = _abi.FAM_GLSZM
for _n in NGTDM:
    FAMILY_OF[_n] = _abi.FAM_NGTDM
for _n in GLDZM:
    FAMILY_OF[_n] = _abi.FAM_GLDZM
for _n in GLDM:
    FAMILY_OF[_n] = _abi.FAM_GLDM
for _n in NGLDM:
    FAMILY_OF[_n] = _abi.FAM_NGLDM
for _n in SMOMS:
    FAMILY_OF[_n] = _abi.FAM_SMOMS
for _n in IMOMS:
    FAMILY_OF[_n] = _abi.FAM_IMOMS
FAMILY_OF["GABOR"] = _abi.FAM_GABOR
# RadialDistributionFeature: three codes of RADIAL_BINS values each (radial_distribution.h:36-39)
RADIAL = ["FRAC_AT_D", "MEAN_FRAC", "RADIAL_CV"]
RADIAL_BINS = 8
for _n in RADIAL:
    FAMILY_OF[_n] = _abi.FAM_RADIAL
FAMILY_OF["ZERNIKE2D"] = _abi.FAM_ZERNIKE
# three classes of the shape block (featureset.h:46-160): one column per code, between the intensity block and GLCM_ASM
FRACTAL = ["FRACT_DIM_BOXCOUNT", "FRACT_DIM_PERIMETER"]
EULER = ["EULER_NUMBER"]
ROI_RADIUS = ["ROI_RADIUS_MEAN", "ROI_RADIUS_MAX", "ROI_RADIUS_MEDIAN"]
for _n in FRACTAL:
    FAMILY_OF[_n] = _abi.FAM_FRACTAL
for _n in EULER:
    FAMILY_OF[_n] = _abi.FAM_EULER
for _n in ROI_RADIUS:
    FAMILY_OF[_n] = _abi.FAM_ROI_RADIUS

# the three caliper classes (featureset.h:93-114): between FRACT_DIM_PERIMETER and EULER_NUMBER.  No group token: the reference's
# tokens that cover these codes also cover codes the path does not serve.
_STAT6 = ["MIN", "MAX", "MEAN", "MEDIAN", "STDDEV", "MODE"]
FERET = ["MIN_FERET_ANGLE", "MAX_FERET_ANGLE"] + ["STAT_FERET_DIAM_" + k for k in _STAT6]
MARTIN = ["STAT_MARTIN_DIAM_" + k for k in _STAT6]
NASSENSTEIN = ["STAT_NASSENSTEIN_DIAM_" + k for k in _STAT6]
for _n in FERET:
    FAMILY_OF[_n] = _abi.FAM_FERET
for _n in MARTIN:
    FAMILY_OF[_n] = _abi.FAM_MARTIN
for _n in NASSENSTEIN:
    FAMILY_OF[_n] = _abi.FAM_NASSENSTEIN

# ChordsFeature (featureset.h:117-132): between STAT_NASSENSTEIN_DIAM_MODE and EULER_NUMBER.  No group token, for the same reason.
_STAT8 = ["MAX", "MAX_ANG", "MIN", "MIN_ANG", "MEDIAN", "MEAN", "MODE", "STDDEV"]
CHORDS = ["MAXCHORDS_" + k for k in _STAT8] + ["ALLCHORDS_" + k for k in _STAT8]
for _n in CHORDS:
    FAMILY_OF[_n] = _abi.FAM_CHORDS

# EllipseFittingFeature and ErosionPixelsFeature (featureset.h:62-68, :85-86): directly behind the intensity block, in front of
# FRACT_DIM_BOXCOUNT.  No group token, for the same reason.
ELLIPSE = ["MAJOR_AXIS_LENGTH", "MINOR_AXIS_LENGTH", "ELONGATION", "ECCENTRICITY", "ORIENTATION", "ROUNDNESS"]
EROSION = ["EROSIONS_2_VANISH", "EROSIONS_2_VANISH_COMPLEMENT"]
for _n in ELLIPSE:
    FAMILY_OF[_n] = _abi.FAM_ELLIPSE
for _n in EROSION:
    FAMILY_OF[_n] = _abi.FAM_EROSION

# EnclosingInscribingCircumscribingCircleFeature and GeodeticLengthThicknessFeature (featureset.h:150-155): directly behind
# EULER_NUMBER, in front of ROI_RADIUS_MEAN.  No group token, for the same reason.
CIRCLES = ["DIAMETER_MIN_ENCLOSING_CIRCLE", "DIAMETER_CIRCUMSCRIBING_CIRCLE", "DIAMETER_INSCRIBING_CIRCLE"]
GEODETIC = ["GEODETIC_LENGTH", "THICKNESS"]
for _n in CIRCLES:
    FAMILY_OF[_n] = _abi.FAM_CIRCLES
for _n in GEODETIC:
    FAMILY_OF[_n] = _abi.FAM_GEODETIC

# NeighborsFeature (featureset.h:162-171): behind ROI_RADIUS_MEDIAN, in front of GLCM_ASM.  The class relates the ROIs of an image to each
# other, so it is no family of the C ABI's mask: FAM_NEIGHBORS is a marker of this module alone (bit 32: beyond the 32-bit mask, it never
# crosses the ABI -- split_neighbors() takes it off) that sends a call to the neighbor entries (nyxhip_neighbors_tiles).
NEIGHBORS = ["NUM_NEIGHBORS", "PERCENT_TOUCHING", "CLOSEST_NEIGHBOR1_DIST", "CLOSEST_NEIGHBOR1_ANG", "CLOSEST_NEIGHBOR2_DIST",
             "CLOSEST_NEIGHBOR2_ANG", "ANG_BW_NEIGHBORS_MEAN", "ANG_BW_NEIGHBORS_STDDEV", "ANG_BW_NEIGHBORS_MODE"]
FAM_NEIGHBORS = 1 << 32
for _n in NEIGHBORS:
    FAMILY_OF[_n] = FAM_NEIGHBORS

# IntensityHistogramFeatures (featureset.h:584-637): the 46 IBSI intensity-histogram codes at the very end of Feature2D, behind IMOM_WHU7.  Like
# the neighbor class it is no family of the C ABI's mask (every bit is spoken for): FAM_IH is a marker of this module alone (bit 33, it never
# crosses the ABI -- split_neighbors() takes it off, split_ih() reads it) that sends a call to the entries of its own (nyxhip_ih_tiles).
# The class exists in IBSI mode only: with `ibsi` off the codes are dropped at call time (env_features.cpp:516-527; nyxus.py).
_IH_STATS = ["MEAN", "VARIANCE", "SKEWNESS", "EXCESS_KURTOSIS", "MEDIAN", "MINIMUM", "P10", "P90", "MAXIMUM", "MODE", "INTERQUANTILE_RANGE", "RANGE",
             "MEAN_ABSOLUTE_DEVIATION", "ROBUST_MEAN_ABSOLUTE_DEVIATION", "MEDIAN_ABSOLUTE_DEVIATION", "COEFFICIENT_OF_VARIATION",
             "QUANTILE_COEFFICIENT_OF_DISPERSION", "ENTROPY", "UNIFORMITY"]
IH = (["IH_%s_VAL" % k for k in _IH_STATS] + ["IH_ROBUST_MEAN_VAL"] + ["IH_%s_IDX" % k for k in _IH_STATS]
      + ["IH_MAX_GRADIENT", "IH_MAX_GRADIENT_IDX", "IH_MIN_GRADIENT", "IH_MIN_GRADIENT_IDX", "IH_ROBUST_MEAN_IDX", "IH_NUM_BINS", "IH_BIN_SIZE"])
FAM_IH = 1 << 33
for _n in IH:
    FAMILY_OF[_n] = FAM_IH


def split_ih(mask: int) -> bool:
    """Whether the intensity-histogram marker is set."""
    return bool(mask & FAM_IH)


def split_neighbors(mask: int) -> Tuple[int, bool]:
    """(the family mask of the C ABI, whether the neighbor marker was set)."""
    return mask & 0xFFFFFFFF, bool(mask & FAM_NEIGHBORS)


# group tokens (featureset.cpp:650-665) the HIP path can serve completely (the radial distribution has none, featureset.cpp:650-668)
GROUPS: Dict[str, List[str]] = {
    "*ALL_INTENSITY*": INTENSITY,
    "*ALL_GLCM*": GLCM_ANGLED + GLCM_AVE,
    "*ALL_GLRLM*": GLRLM_ANGLED + GLRLM_AVE,
    "*ALL_GLDZM*": GLDZM,
    "*ALL_GLSZM*": GLSZM,
    "*ALL_GLDM*": GLDM,
    "*ALL_NGLDM*": NGLDM,
    "*ALL_NGTDM*": NGTDM,
    "*GEOMOMS*": SMOMS + IMOMS,      # env_features.cpp:316-333
    "*SGEOMOMS*": SMOMS,
    "*IGEOMOMS*": IMOMS,
    "*ALL_NEIGHBOR*": NEIGHBORS,
    "*ALL_IH*": IH,                  # FG2_IH; served in IBSI mode only
}

# enum order of every feature code the path covers (one entry per Feature2D code)
ENUM_ORDER: List[str] = (INTENSITY + GLCM_ANGLED + GLCM_AVE + GLRLM_ANGLED + GLRLM_AVE + GLDZM + GLSZM + GLDM + NGLDM + NGTDM
                         + ["FRAC_AT_D", "GABOR", "MEAN_FRAC", "RADIAL_CV", "ZERNIKE2D"] + SMOMS + IMOMS)   # featureset.h:352-357
# ... and the order expand() returns codes in: ENUM_ORDER with the shape-block codes at their enum position (ENUM_ORDER itself
# keeps the codes of the twelve FAM_ALL families and the radial distribution)
OUTPUT_ORDER: List[str] = INTENSITY + FRACTAL + EULER + ROI_RADIUS + ENUM_ORDER[len(INTENSITY):]
# every served code in true enum order: OUTPUT_ORDER with the caliper codes behind FRACT_DIM_PERIMETER.
SERVED_ORDER: List[str] = INTENSITY + FRACTAL + FERET + MARTIN + NASSENSTEIN + OUTPUT_ORDER[len(INTENSITY) + len(FRACTAL):]
# ... and SERVED_ORDER with the chords codes behind STAT_NASSENSTEIN_DIAM_MODE (SERVED_ORDER keeps the codes it was introduced with,
# like ENUM_ORDER and OUTPUT_ORDER before it).
_K = len(INTENSITY) + len(FRACTAL) + len(FERET) + len(MARTIN) + len(NASSENSTEIN)
CATALOGUE_ORDER: List[str] = SERVED_ORDER[:_K] + CHORDS + SERVED_ORDER[_K:]
# ... and CATALOGUE_ORDER with the ellipse and erosion codes behind the intensity codes (CATALOGUE_ORDER keeps the codes it was
# introduced with, like the three lists before it).
FULL_ORDER: List[str] = INTENSITY + ELLIPSE + EROSION + CATALOGUE_ORDER[len(INTENSITY):]
# ... and FULL_ORDER with the circle and geodetic codes behind EULER_NUMBER (FULL_ORDER keeps the codes it was introduced with, like
# the four lists before it).  expand() orders by this list.
_E = FULL_ORDER.index("EULER_NUMBER") + 1
EXPAND_ORDER: List[str] = FULL_ORDER[:_E] + CIRCLES + GEODETIC + FULL_ORDER[_E:]
# ... and EXPAND_ORDER with the neighbor codes behind ROI_RADIUS_MEDIAN (EXPAND_ORDER keeps the codes it was introduced with, like the
# five lists before it).  expand() orders by this list.
_R = EXPAND_ORDER.index("ROI_RADIUS_MEDIAN") + 1
REQUEST_ORDER: List[str] = EXPAND_ORDER[:_R] + NEIGHBORS + EXPAND_ORDER[_R:]
# ... and REQUEST_ORDER with the intensity-histogram codes behind IMOM_WHU7, the end of the enum (REQUEST_ORDER keeps the codes it was
# introduced with, like the six lists before it).  expand() orders by this list.
IH_REQUEST_ORDER: List[str] = REQUEST_ORDER + IH


def expand(features: List[str]) -> Tuple[int, List[str]]:
    """Expands group tokens, validates names, returns (family mask, requested feature codes in enum order).  The mask holds
    FAM_NEIGHBORS (bit 32, not a bit of the C ABI: split_neighbors) when a neighbor code is among them, and FAM_IH (bit 33, split_ih) when an
    intensity-histogram code is."""
    want = set()
    unknown = []
    for f in features:
        key = f.strip()
        if key.upper() in GROUPS:
            want.update(GROUPS[key.upper()])
        elif key.upper() in FAMILY_OF:
            want.add(key.upper())
        else:
            unknown.append(f)
    if unknown:
        raise ValueError(
            f"feature(s) {unknown} are not served by the MI355X path. Implemented: groups {sorted(GROUPS)} and the "
            f"individual features of the intensity, GLCM, GLRLM, GLDZM, GLSZM, GLDM, NGLDM and NGTDM families, GABOR, ZERNIKE2D, "
            f"FRAC_AT_D, MEAN_FRAC, RADIAL_CV, FRACT_DIM_BOXCOUNT, FRACT_DIM_PERIMETER, EULER_NUMBER, ROI_RADIUS_MEAN, ROI_RADIUS_MAX, "
            f"ROI_RADIUS_MEDIAN, MIN_FERET_ANGLE, MAX_FERET_ANGLE and STAT_{{FERET,MARTIN,NASSENSTEIN}}_DIAM_{{MIN,MAX,MEAN,MEDIAN,STDDEV,MODE}}, "
            f"{{MAXCHORDS,ALLCHORDS}}_{{MAX,MAX_ANG,MIN,MIN_ANG,MEDIAN,MEAN,MODE,STDDEV}}, MAJOR_AXIS_LENGTH, MINOR_AXIS_LENGTH, ELONGATION, "
            f"ECCENTRICITY, ORIENTATION, ROUNDNESS, EROSIONS_2_VANISH, EROSIONS_2_VANISH_COMPLEMENT, DIAMETER_MIN_ENCLOSING_CIRCLE, "
            f"DIAMETER_CIRCUMSCRIBING_CIRCLE, DIAMETER_INSCRIBING_CIRCLE, GEODETIC_LENGTH, THICKNESS, {', '.join(NEIGHBORS)}, "
            f"{', '.join(IH)} (IBSI mode)")
    if not want:
        raise ValueError("no features requested")
    ordered = [n for n in IH_REQUEST_ORDER if n in want]
    mask = 0
    for n in ordered:
        mask |= FAMILY_OF[n]
    return mask, ordered


def column_selector(requested: List[str], all_columns: List[str], glcm_angles: List[int]) -> List[int]:
    """Indices into the library's table (all columns of the touched families) of the columns that belong
    to the requested feature codes, in output order (save_features_2_buffer, output_2_buffer.cpp:316-445)."""
    idx_of = {c: i for i, c in enumerate(all_columns)}
    sel: List[int] = []
    for code in requested:
        if code in GLCM_ANGLED:
            sel += [idx_of[f"{code}_{a}"] for a in glcm_angles]
        elif code in GLRLM_ANGLED:
            sel += [idx_of[f"{code}_{a}"] for a in (0, 45, 90, 135)]
        elif code == "GABOR":
            sel += [i for i, c in enumerate(all_columns) if c.startswith("GABOR_")]
        elif code in RADIAL:
            sel += [idx_of[f"{code}_{i}"] for i in range(RADIAL_BINS)]       # output_2_buffer.cpp:374-411
        elif code == "ZERNIKE2D":
            sel += [i for i, c in enumerate(all_columns) if c.startswith("ZERNIKE2D_Z")]
        else:
            sel.append(idx_of[code])
    return sel
