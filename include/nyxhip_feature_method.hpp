// nyxhip_feature_method.hpp -- the reference's plugin surface, served by the HIP hot path.
//
// A header-only C++ adapter above the C ABI (nyxhip.h) that mirrors, name for name, the pieces of the
// reference a feature plugin touches, so that code written against Nyxus' `FeatureMethod` shape -- and the
// reference's own unit tests (tests/test_2d_*_common.h: build an LR from a pixel list, `f.calculate(r, s)`,
// `f.save_value(r.fvals)`) -- reads the same here:
//
//   Feature2D / FeatureSet      /root/reference/src/nyx/featureset.h:10-641, featureset.cpp:1198
//   NyxSetting / Fsettings      src/nyx/feature_settings.h:6-54
//   Pixel2, AABB, LR            src/nyx/features/pixel.h:52-61, features/aabb.h, roi_cache.h:31-84
//   SlideProps / Dataset        src/nyx/slideprops.h:6-89, dataset.h:6-26
//   FeatureMethod               src/nyx/feature_method.h:11-80   (provide_features, required, calculate, save_value)
//   functype / runParallel      src/nyx/parallel.h:13,23-42      (static F::reduce(start,end,labels,roiData,settings,dataset))
//   reduce_trivial_rois_manual  src/nyx/reduce_trivial_rois.cpp:772-795
//
// Differences, all forced by the boundary: feature codes cover only the seven hot-path families (the enum
// keeps the reference's identifiers and relative order); `calculate()` of ANY family runs the fused kernels
// for that family on the GPU; `osized_*` (out-of-core ROIs) throw -- they are outside SURVEY.md section 8.
// Errors follow the WITH_PYTHON_H convention of the reference: std::runtime_error.
#pragma once
#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <limits>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "nyxhip.h"

namespace NyxusHip {

// ---- feature codes (identifiers and order of Nyxus::Feature2D, hot-path families only) -----------
enum class Feature2D : int {
    COV = 0, COVERED_IMAGE_INTENSITY_RANGE, ENERGY, ENTROPY, EXCESS_KURTOSIS, HYPERFLATNESS, HYPERSKEWNESS,
    INTEGRATED_INTENSITY, INTERQUARTILE_RANGE, KURTOSIS, MAX, MEAN, MEAN_ABSOLUTE_DEVIATION, MEDIAN,
    MEDIAN_ABSOLUTE_DEVIATION, MIN, MODE, P01, P10, P25, P75, P90, P99, QCOD, RANGE, ROBUST_MEAN,
    ROBUST_MEAN_ABSOLUTE_DEVIATION, ROOT_MEAN_SQUARED, SKEWNESS, STANDARD_DEVIATION, STANDARD_DEVIATION_BIASED,
    STANDARD_ERROR, VARIANCE, VARIANCE_BIASED, UNIFORMITY, UNIFORMITY_PIU,
    // three classes of the shape block (featureset.h:46-160), in enum position: between the intensity block and GLCM
    FRACT_DIM_BOXCOUNT, FRACT_DIM_PERIMETER,
    // the caliper classes (featureset.h:93-114)
    MIN_FERET_ANGLE, MAX_FERET_ANGLE, STAT_FERET_DIAM_MIN, STAT_FERET_DIAM_MAX, STAT_FERET_DIAM_MEAN, STAT_FERET_DIAM_MEDIAN, STAT_FERET_DIAM_STDDEV,
    STAT_FERET_DIAM_MODE, STAT_MARTIN_DIAM_MIN, STAT_MARTIN_DIAM_MAX, STAT_MARTIN_DIAM_MEAN, STAT_MARTIN_DIAM_MEDIAN, STAT_MARTIN_DIAM_STDDEV,
    STAT_MARTIN_DIAM_MODE, STAT_NASSENSTEIN_DIAM_MIN, STAT_NASSENSTEIN_DIAM_MAX, STAT_NASSENSTEIN_DIAM_MEAN, STAT_NASSENSTEIN_DIAM_MEDIAN,
    STAT_NASSENSTEIN_DIAM_STDDEV, STAT_NASSENSTEIN_DIAM_MODE,
    EULER_NUMBER, ROI_RADIUS_MEAN, ROI_RADIUS_MAX, ROI_RADIUS_MEDIAN,
    GLCM_ASM, GLCM_ACOR, GLCM_CLUPROM, GLCM_CLUSHADE, GLCM_CLUTEND, GLCM_CONTRAST, GLCM_CORRELATION, GLCM_DIFAVE,
    GLCM_DIFENTRO, GLCM_DIFVAR, GLCM_DIS, GLCM_ENERGY, GLCM_ENTROPY, GLCM_HOM1, GLCM_HOM2, GLCM_ID, GLCM_IDN,
    GLCM_IDM, GLCM_IDMN, GLCM_INFOMEAS1, GLCM_INFOMEAS2, GLCM_IV, GLCM_JAVE, GLCM_JE, GLCM_JMAX, GLCM_JVAR,
    GLCM_SUMAVERAGE, GLCM_SUMENTROPY, GLCM_SUMVARIANCE, GLCM_VARIANCE,
    GLCM_ASM_AVE, GLCM_ACOR_AVE, GLCM_CLUPROM_AVE, GLCM_CLUSHADE_AVE, GLCM_CLUTEND_AVE, GLCM_CONTRAST_AVE,
    GLCM_CORRELATION_AVE, GLCM_DIFAVE_AVE, GLCM_DIFENTRO_AVE, GLCM_DIFVAR_AVE, GLCM_DIS_AVE, GLCM_ENERGY_AVE,
    GLCM_ENTROPY_AVE, GLCM_HOM1_AVE, GLCM_ID_AVE, GLCM_IDN_AVE, GLCM_IDM_AVE, GLCM_IDMN_AVE, GLCM_IV_AVE,
    GLCM_JAVE_AVE, GLCM_JE_AVE, GLCM_INFOMEAS1_AVE, GLCM_INFOMEAS2_AVE, GLCM_VARIANCE_AVE, GLCM_JMAX_AVE,
    GLCM_JVAR_AVE, GLCM_SUMAVERAGE_AVE, GLCM_SUMENTROPY_AVE, GLCM_SUMVARIANCE_AVE,
    GLRLM_SRE, GLRLM_LRE, GLRLM_GLN, GLRLM_GLNN, GLRLM_RLN, GLRLM_RLNN, GLRLM_RP, GLRLM_GLV, GLRLM_RV, GLRLM_RE,
    GLRLM_LGLRE, GLRLM_HGLRE, GLRLM_SRLGLE, GLRLM_SRHGLE, GLRLM_LRLGLE, GLRLM_LRHGLE,
    GLRLM_SRE_AVE, GLRLM_LRE_AVE, GLRLM_GLN_AVE, GLRLM_GLNN_AVE, GLRLM_RLN_AVE, GLRLM_RLNN_AVE, GLRLM_RP_AVE,
    GLRLM_GLV_AVE, GLRLM_RV_AVE, GLRLM_RE_AVE, GLRLM_LGLRE_AVE, GLRLM_HGLRE_AVE, GLRLM_SRLGLE_AVE,
    GLRLM_SRHGLE_AVE, GLRLM_LRLGLE_AVE, GLRLM_LRHGLE_AVE,
    GLDZM_SDE, GLDZM_LDE, GLDZM_LGLZE, GLDZM_HGLZE, GLDZM_SDLGLE, GLDZM_SDHGLE, GLDZM_LDLGLE, GLDZM_LDHGLE, GLDZM_GLNU,
    GLDZM_GLNUN, GLDZM_ZDNU, GLDZM_ZDNUN, GLDZM_ZP, GLDZM_GLM, GLDZM_GLV, GLDZM_ZDM, GLDZM_ZDV, GLDZM_ZDE,
    GLSZM_SAE, GLSZM_LAE, GLSZM_GLN, GLSZM_GLNN, GLSZM_SZN, GLSZM_SZNN, GLSZM_ZP, GLSZM_GLV, GLSZM_ZV, GLSZM_ZE,
    GLSZM_LGLZE, GLSZM_HGLZE, GLSZM_SALGLE, GLSZM_SAHGLE, GLSZM_LALGLE, GLSZM_LAHGLE,
    GLDM_SDE, GLDM_LDE, GLDM_GLN, GLDM_DN, GLDM_DNN, GLDM_GLV, GLDM_DV, GLDM_DE, GLDM_LGLE, GLDM_HGLE, GLDM_SDLGLE,
    GLDM_SDHGLE, GLDM_LDLGLE, GLDM_LDHGLE,
    NGLDM_LDE, NGLDM_HDE, NGLDM_LGLCE, NGLDM_HGLCE, NGLDM_LDLGLE, NGLDM_LDHGLE, NGLDM_HDLGLE, NGLDM_HDHGLE, NGLDM_GLNU,
    NGLDM_GLNUN, NGLDM_DCNU, NGLDM_DCNUN, NGLDM_DCP, NGLDM_GLM, NGLDM_GLV, NGLDM_DCM, NGLDM_DCV, NGLDM_DCENT, NGLDM_DCENE,
    NGTDM_COARSENESS, NGTDM_CONTRAST, NGTDM_BUSYNESS, NGTDM_COMPLEXITY, NGTDM_STRENGTH,
    FRAC_AT_D, GABOR, MEAN_FRAC, RADIAL_CV, ZERNIKE2D,      // featureset.h:352-357: the radial distribution interleaves with Gabor
    // shape / intensity geometric moments (featureset.h:362-565)
    SPAT_MOMENT_00, SPAT_MOMENT_01, SPAT_MOMENT_02, SPAT_MOMENT_03, SPAT_MOMENT_10, SPAT_MOMENT_11, SPAT_MOMENT_12,
    SPAT_MOMENT_13, SPAT_MOMENT_20, SPAT_MOMENT_21, SPAT_MOMENT_22, SPAT_MOMENT_23, SPAT_MOMENT_30, CENTRAL_MOMENT_00,
    CENTRAL_MOMENT_01, CENTRAL_MOMENT_02, CENTRAL_MOMENT_03, CENTRAL_MOMENT_10, CENTRAL_MOMENT_11, CENTRAL_MOMENT_12,
    CENTRAL_MOMENT_13, CENTRAL_MOMENT_20, CENTRAL_MOMENT_21, CENTRAL_MOMENT_22, CENTRAL_MOMENT_23, CENTRAL_MOMENT_30,
    CENTRAL_MOMENT_31, CENTRAL_MOMENT_32, CENTRAL_MOMENT_33, NORM_SPAT_MOMENT_00, NORM_SPAT_MOMENT_01,
    NORM_SPAT_MOMENT_02, NORM_SPAT_MOMENT_03, NORM_SPAT_MOMENT_10, NORM_SPAT_MOMENT_11, NORM_SPAT_MOMENT_12,
    NORM_SPAT_MOMENT_13, NORM_SPAT_MOMENT_20, NORM_SPAT_MOMENT_21, NORM_SPAT_MOMENT_22, NORM_SPAT_MOMENT_23,
    NORM_SPAT_MOMENT_30, NORM_SPAT_MOMENT_31, NORM_SPAT_MOMENT_32, NORM_SPAT_MOMENT_33, NORM_CENTRAL_MOMENT_02,
    NORM_CENTRAL_MOMENT_03, NORM_CENTRAL_MOMENT_11, NORM_CENTRAL_MOMENT_12, NORM_CENTRAL_MOMENT_20,
    NORM_CENTRAL_MOMENT_21, NORM_CENTRAL_MOMENT_30, HU_M1, HU_M2, HU_M3, HU_M4, HU_M5, HU_M6, HU_M7,
    WEIGHTED_SPAT_MOMENT_00, WEIGHTED_SPAT_MOMENT_01, WEIGHTED_SPAT_MOMENT_02, WEIGHTED_SPAT_MOMENT_03,
    WEIGHTED_SPAT_MOMENT_10, WEIGHTED_SPAT_MOMENT_11, WEIGHTED_SPAT_MOMENT_12, WEIGHTED_SPAT_MOMENT_20,
    WEIGHTED_SPAT_MOMENT_21, WEIGHTED_SPAT_MOMENT_30, WEIGHTED_CENTRAL_MOMENT_02, WEIGHTED_CENTRAL_MOMENT_03,
    WEIGHTED_CENTRAL_MOMENT_11, WEIGHTED_CENTRAL_MOMENT_12, WEIGHTED_CENTRAL_MOMENT_20, WEIGHTED_CENTRAL_MOMENT_21,
    WEIGHTED_CENTRAL_MOMENT_30, WT_NORM_CTR_MOM_02, WT_NORM_CTR_MOM_03, WT_NORM_CTR_MOM_11, WT_NORM_CTR_MOM_12,
    WT_NORM_CTR_MOM_20, WT_NORM_CTR_MOM_21, WT_NORM_CTR_MOM_30, WEIGHTED_HU_M1, WEIGHTED_HU_M2, WEIGHTED_HU_M3,
    WEIGHTED_HU_M4, WEIGHTED_HU_M5, WEIGHTED_HU_M6, WEIGHTED_HU_M7,
    IMOM_RM_00, IMOM_RM_01, IMOM_RM_02, IMOM_RM_03, IMOM_RM_10, IMOM_RM_11, IMOM_RM_12, IMOM_RM_13, IMOM_RM_20,
    IMOM_RM_21, IMOM_RM_22, IMOM_RM_23, IMOM_RM_30, IMOM_CM_00, IMOM_CM_01, IMOM_CM_02, IMOM_CM_03, IMOM_CM_10,
    IMOM_CM_11, IMOM_CM_12, IMOM_CM_13, IMOM_CM_20, IMOM_CM_21, IMOM_CM_22, IMOM_CM_23, IMOM_CM_30, IMOM_CM_31,
    IMOM_CM_32, IMOM_CM_33, IMOM_NRM_00, IMOM_NRM_01, IMOM_NRM_02, IMOM_NRM_03, IMOM_NRM_10, IMOM_NRM_11, IMOM_NRM_12,
    IMOM_NRM_13, IMOM_NRM_20, IMOM_NRM_21, IMOM_NRM_22, IMOM_NRM_23, IMOM_NRM_30, IMOM_NRM_31, IMOM_NRM_32,
    IMOM_NRM_33, IMOM_NCM_02, IMOM_NCM_03, IMOM_NCM_11, IMOM_NCM_12, IMOM_NCM_20, IMOM_NCM_21, IMOM_NCM_30, IMOM_HU1,
    IMOM_HU2, IMOM_HU3, IMOM_HU4, IMOM_HU5, IMOM_HU6, IMOM_HU7, IMOM_WRM_00, IMOM_WRM_01, IMOM_WRM_02, IMOM_WRM_03,
    IMOM_WRM_10, IMOM_WRM_11, IMOM_WRM_12, IMOM_WRM_20, IMOM_WRM_21, IMOM_WRM_30, IMOM_WCM_02, IMOM_WCM_03,
    IMOM_WCM_11, IMOM_WCM_12, IMOM_WCM_20, IMOM_WCM_21, IMOM_WCM_30, IMOM_WNCM_02, IMOM_WNCM_03, IMOM_WNCM_11,
    IMOM_WNCM_12, IMOM_WNCM_20, IMOM_WNCM_21, IMOM_WNCM_30, IMOM_WHU1, IMOM_WHU2, IMOM_WHU3, IMOM_WHU4, IMOM_WHU5,
    IMOM_WHU6, IMOM_WHU7,
    // ChordsFeature (featureset.h:117-132).  In the reference these sixteen sit between STAT_NASSENSTEIN_DIAM_MODE and EULER_NUMBER, and
    // that is where their table columns are; this mirror numbers them last, so that the codes it had before keep their neighbours.
    MAXCHORDS_MAX, MAXCHORDS_MAX_ANG, MAXCHORDS_MIN, MAXCHORDS_MIN_ANG, MAXCHORDS_MEDIAN, MAXCHORDS_MEAN, MAXCHORDS_MODE, MAXCHORDS_STDDEV,
    ALLCHORDS_MAX, ALLCHORDS_MAX_ANG, ALLCHORDS_MIN, ALLCHORDS_MIN_ANG, ALLCHORDS_MEDIAN, ALLCHORDS_MEAN, ALLCHORDS_MODE, ALLCHORDS_STDDEV,
    // EllipseFittingFeature (featureset.h:62-68) and ErosionPixelsFeature (:85-86).  In the reference these eight sit behind the intensity
    // block, in front of FRACT_DIM_BOXCOUNT, and that is where their table columns are; numbered last here for the same reason.
    MAJOR_AXIS_LENGTH, MINOR_AXIS_LENGTH, ELONGATION, ECCENTRICITY, ORIENTATION, ROUNDNESS,
    EROSIONS_2_VANISH, EROSIONS_2_VANISH_COMPLEMENT,
    // EnclosingInscribingCircumscribingCircleFeature (featureset.h:150-152) and GeodeticLengthThicknessFeature (:154-155).  In the
    // reference these five sit behind EULER_NUMBER, in front of ROI_RADIUS_MEAN, and that is where their table columns are; numbered
    // last here for the same reason.
    DIAMETER_MIN_ENCLOSING_CIRCLE, DIAMETER_CIRCUMSCRIBING_CIRCLE, DIAMETER_INSCRIBING_CIRCLE,
    GEODETIC_LENGTH, THICKNESS,
    // NeighborsFeature (featureset.h:162-171).  In the reference these nine sit behind ROI_RADIUS_MEDIAN, in front of GLCM_ASM, and that is
    // where the Python face puts their columns; numbered last here for the same reason.
    NUM_NEIGHBORS, PERCENT_TOUCHING, CLOSEST_NEIGHBOR1_DIST, CLOSEST_NEIGHBOR1_ANG, CLOSEST_NEIGHBOR2_DIST, CLOSEST_NEIGHBOR2_ANG,
    ANG_BW_NEIGHBORS_MEAN, ANG_BW_NEIGHBORS_STDDEV, ANG_BW_NEIGHBORS_MODE,
    // IntensityHistogramFeatures (featureset.h:584-637): the 46 IBSI intensity-histogram codes.  Numbered last here -- which, for once, is
    // also their true position: the reference appended them to Feature2D so that no existing code shifts.
    IH_MEAN_VAL, IH_VARIANCE_VAL, IH_SKEWNESS_VAL, IH_EXCESS_KURTOSIS_VAL, IH_MEDIAN_VAL, IH_MINIMUM_VAL, IH_P10_VAL, IH_P90_VAL, IH_MAXIMUM_VAL,
    IH_MODE_VAL, IH_INTERQUANTILE_RANGE_VAL, IH_RANGE_VAL, IH_MEAN_ABSOLUTE_DEVIATION_VAL, IH_ROBUST_MEAN_ABSOLUTE_DEVIATION_VAL,
    IH_MEDIAN_ABSOLUTE_DEVIATION_VAL, IH_COEFFICIENT_OF_VARIATION_VAL, IH_QUANTILE_COEFFICIENT_OF_DISPERSION_VAL, IH_ENTROPY_VAL,
    IH_UNIFORMITY_VAL, IH_ROBUST_MEAN_VAL,
    IH_MEAN_IDX, IH_VARIANCE_IDX, IH_SKEWNESS_IDX, IH_EXCESS_KURTOSIS_IDX, IH_MEDIAN_IDX, IH_MINIMUM_IDX, IH_P10_IDX, IH_P90_IDX, IH_MAXIMUM_IDX,
    IH_MODE_IDX, IH_INTERQUANTILE_RANGE_IDX, IH_RANGE_IDX, IH_MEAN_ABSOLUTE_DEVIATION_IDX, IH_ROBUST_MEAN_ABSOLUTE_DEVIATION_IDX,
    IH_MEDIAN_ABSOLUTE_DEVIATION_IDX, IH_COEFFICIENT_OF_VARIATION_IDX, IH_QUANTILE_COEFFICIENT_OF_DISPERSION_IDX, IH_ENTROPY_IDX,
    IH_UNIFORMITY_IDX,
    IH_MAX_GRADIENT, IH_MAX_GRADIENT_IDX, IH_MIN_GRADIENT, IH_MIN_GRADIENT_IDX, IH_ROBUST_MEAN_IDX, IH_NUM_BINS, IH_BIN_SIZE,
    _COUNT_
};

// The image-quality codes (featureset.h:920-931): an enum of their own whose values continue behind the other feature enums, so that they
// index the same LR::fvals.  All six are named, as in the reference; FocusScoreFeature and SaturationFeature serve four of them.
// POWER_SPECTRUM_SLOPE and SHARPNESS have no class here (include/nyxhip.h says why).
enum class FeatureIMQ : int {
    FOCUS_SCORE = (int)Feature2D::_COUNT_, LOCAL_FOCUS_SCORE, POWER_SPECTRUM_SLOPE, MAX_SATURATION, MIN_SATURATION, SHARPNESS,
    _COUNT_,
    _FIRST_ = FOCUS_SCORE
};

// POLYGONALITY_AVE, HEXAGONALITY_AVE, HEXAGONALITY_STDDEV (featureset.h:146-148, in the reference between EXTREMA_P8_Y and
// DIAMETER_MIN_ENCLOSING_CIRCLE): an enum of their own whose values continue behind FeatureIMQ, so that they index the same LR::fvals
// and the codes numbered before them keep their values.
enum class FeatureHexPoly : int {
    POLYGONALITY_AVE = (int)FeatureIMQ::_COUNT_, HEXAGONALITY_AVE, HEXAGONALITY_STDDEV,
    _COUNT_,
    _FIRST_ = POLYGONALITY_AVE
};

// ---- settings (feature_settings.h:6-54) ----------------------------------------------------------
union FeatureSetting { bool bval; int ival; double rval; };
typedef std::vector<FeatureSetting> Fsettings;
enum class NyxSetting : int { SOFTNAN = 0, TINY, SINGLEROI, GREYDEPTH, PIXELSIZEUM, PIXELDISTANCE, XYRES, USEGPU, VERBOSLVL, IBSI,
                              GLCM_GREYDEPTH, GLCM_OFFSET, GLCM_NUMANG, __COUNT__ };
#define NYXHIP_STNGS_MISSING(obj) ((int)(obj).size() < (int)NyxusHip::NyxSetting::__COUNT__)

// ---- ROI record (roi_cache.h:31-84) ---------------------------------------------------------------
using PixIntens = unsigned int;
using StatsInt = long;
struct Pixel2 { StatsInt x, y; PixIntens inten; Pixel2(StatsInt x_ = 0, StatsInt y_ = 0, PixIntens i_ = 0) : x(x_), y(y_), inten(i_) {} };

class AABB {
public:
    void init_x(StatsInt x) { xmin = xmax = x; }
    void init_y(StatsInt y) { ymin = ymax = y; }
    void update_x(StatsInt x) { xmin = std::min(xmin, x); xmax = std::max(xmax, x); }
    void update_y(StatsInt y) { ymin = std::min(ymin, y); ymax = std::max(ymax, y); }
    StatsInt get_height() const { return ymax - ymin + 1; }
    StatsInt get_width() const { return xmax - xmin + 1; }
    StatsInt get_xmin() const { return xmin; }
    StatsInt get_ymin() const { return ymin; }
private:
    StatsInt xmin = std::numeric_limits<StatsInt>::max(), xmax = std::numeric_limits<StatsInt>::min(),
             ymin = std::numeric_limits<StatsInt>::max(), ymax = std::numeric_limits<StatsInt>::min();
};

class LR {
public:
    LR(int roi_label = -1) : label(roi_label) {}
    int label;
    int slide_idx = -1;
    std::vector<Pixel2> raw_pixels;
    unsigned int aux_area = 0;
    PixIntens aux_min = (std::numeric_limits<PixIntens>::max)(), aux_max = 0;
    AABB aabb;
    std::vector<std::vector<double>> fvals;
    void initialize_fvals() { fvals.assign((size_t)FeatureHexPoly::_COUNT_, std::vector<double>(1, 0.0)); }   // roi_cache.cpp:105-110
    // phase-1 bookkeeping of one pixel (feed_pixel_2_metrics, pixel_feed.cpp:19-43 + feed_pixel_2_cache :71-74)
    void feed_pixel(StatsInt x, StatsInt y, PixIntens i)
    {
        if (aux_area == 0) { aabb.init_x(x); aabb.init_y(y); } else { aabb.update_x(x); aabb.update_y(y); }
        aux_area++;
        aux_min = std::min(aux_min, i);
        aux_max = std::max(aux_max, i);
        raw_pixels.push_back(Pixel2(x, y, i));
    }
};

struct SlideProps { double min_preroi_inten = -1, max_preroi_inten = -1; };
struct Dataset { std::vector<SlideProps> dataset_props; };

// ---- feature-set bits (featureset.h FeatureSet) ------------------------------------------------------
class FeatureSet {
public:
    FeatureSet() : bits((size_t)FeatureHexPoly::_COUNT_, false) {}
    void enableFeature(FeatureHexPoly f) { bits[(size_t)f] = true; }
    bool isEnabled(FeatureHexPoly f) const { return bits[(size_t)f]; }
    bool anyEnabled(const std::initializer_list<FeatureHexPoly>& F) const { for (auto f : F) if (bits[(size_t)f]) return true; return false; }
    void enableFeature(Feature2D f) { bits[(size_t)f] = true; }
    void enableFeature(FeatureIMQ f) { bits[(size_t)f] = true; }
    void enableFeatures(const std::initializer_list<FeatureIMQ>& F) { for (auto f : F) bits[(size_t)f] = true; }
    bool isEnabled(FeatureIMQ f) const { return bits[(size_t)f]; }
    bool anyEnabled(const std::initializer_list<FeatureIMQ>& F) const { for (auto f : F) if (bits[(size_t)f]) return true; return false; }
    void enableFeatures(const std::initializer_list<Feature2D>& F) { for (auto f : F) bits[(size_t)f] = true; }
    bool isEnabled(Feature2D f) const { return bits[(size_t)f]; }
    bool anyEnabled(const std::initializer_list<Feature2D>& F) const { for (auto f : F) if (bits[(size_t)f]) return true; return false; }
    bool anyEnabledInRange(Feature2D a, Feature2D b) const { for (int i = (int)a; i <= (int)b; i++) if (bits[(size_t)i]) return true; return false; }
private:
    std::vector<bool> bits;
};

// ---- one process-wide device context ------------------------------------------------------------------
inline nyxhip_ctx* context(int device = 0)
{
    static nyxhip_ctx* ctx = nullptr;
    if (!ctx && nyxhip_init(device, &ctx) != NYXHIP_OK)
        throw std::runtime_error(std::string("nyxhip_init: ") + nyxhip_last_error(nullptr));
    return ctx;
}

// Process-global knobs the reference keeps as class statics (glcm.cpp:8-9, gabor.cpp:14-25)
struct Knobs {
    std::vector<int> glcm_angles{0, 45, 90, 135};
    bool symmetric_glcm = false;
    double gabor_gamma = 0.1, gabor_sig2lam = 0.8, gabor_f0LP = 0.1, gabor_GRAYthr = 0.025;
    int gabor_n = 16;
    std::vector<std::pair<double, double>> f0_theta_pairs{{0, 4.0}, {0.78539816339744830962, 16.0}, {1.57079632679489661923, 32.0}, {0.78539816339744830962 * 3.0, 64.0}};
};
inline Knobs& knobs() { static Knobs k; return k; }

inline nyxhip_settings make_settings(const Fsettings& s)
{
    nyxhip_settings o;
    nyxhip_default_settings(&o);
    const Knobs& k = knobs();
    if (NYXHIP_STNGS_MISSING(s)) {
        o.grey_depth = 24;                                 // DEFAULT_NUM_HISTO_BINS when settings are missing (intensity.cpp:125)
        o.glcm_grey_depth = 24;
    } else {
        o.soft_nan = s[(int)NyxSetting::SOFTNAN].rval;
        o.tiny = s[(int)NyxSetting::TINY].rval;
        o.grey_depth = s[(int)NyxSetting::GREYDEPTH].ival;
        o.ibsi = s[(int)NyxSetting::IBSI].bval ? 1 : 0;
        o.glcm_grey_depth = s[(int)NyxSetting::GLCM_GREYDEPTH].ival;
        o.glcm_offset = s[(int)NyxSetting::GLCM_OFFSET].ival;
        if (o.ibsi && o.grey_depth == 0) o.grey_depth = 1; // histogram bins are irrelevant to the IBSI texture paths
    }
    o.glcm_n_angles = (int)k.glcm_angles.size();
    for (int i = 0; i < o.glcm_n_angles; i++) o.glcm_angles[i] = k.glcm_angles[i];
    o.glcm_symmetric = k.symmetric_glcm ? 1 : 0;
    o.gabor_gamma = k.gabor_gamma; o.gabor_sig2lam = k.gabor_sig2lam; o.gabor_f0lp = k.gabor_f0LP; o.gabor_graythr = k.gabor_GRAYthr;
    o.gabor_kersize = k.gabor_n; o.gabor_n_filters = (int)k.f0_theta_pairs.size();
    for (int i = 0; i < o.gabor_n_filters; i++) { o.gabor_f0[i] = k.f0_theta_pairs[i].first; o.gabor_theta[i] = k.f0_theta_pairs[i].second; }
    return o;
}

// Gathers labels[start,end) into the SoA batch, runs the families of `mask`, scatters into LR::fvals.
inline void reduce_range(uint32_t mask, size_t start, size_t end, std::vector<int>* labels, std::unordered_map<int, LR>* roiData,
                         const Fsettings& fst, const Dataset& ds)
{
    if (end <= start) return;
    nyxhip_settings s = make_settings(fst);
    const size_t n = end - start;
    std::vector<uint32_t> lab(n), bw(n), bh(n), mn(n), mx(n), ox(n), oy(n), inten;
    std::vector<uint64_t> off(n + 1, 0);
    std::vector<uint16_t> x, y;
    std::vector<double> smin(n), smax(n);
    bool have_slide = true;
    for (size_t i = 0; i < n; i++) {
        LR& r = (*roiData)[(*labels)[start + i]];
        lab[i] = (uint32_t)r.label; bw[i] = (uint32_t)r.aabb.get_width(); bh[i] = (uint32_t)r.aabb.get_height();
        mn[i] = r.aux_min; mx[i] = r.aux_max;
        ox[i] = (uint32_t)r.aabb.get_xmin(); oy[i] = (uint32_t)r.aabb.get_ymin();   // the ROI's position (read by the caliper classes, the chords and the circle class)
        for (const Pixel2& p : r.raw_pixels) { x.push_back((uint16_t)(p.x - r.aabb.get_xmin())); y.push_back((uint16_t)(p.y - r.aabb.get_ymin())); inten.push_back(p.inten); }
        off[i + 1] = inten.size();
        if (r.slide_idx >= 0 && (size_t)r.slide_idx < ds.dataset_props.size()) { smin[i] = ds.dataset_props[r.slide_idx].min_preroi_inten; smax[i] = ds.dataset_props[r.slide_idx].max_preroi_inten; }
        else have_slide = false;
        if (r.fvals.empty()) r.initialize_fvals();
    }
    nyxhip_batch b{};
    b.n_roi = n; b.roi_label = lab.data(); b.px_offset = off.data(); b.x = x.data(); b.y = y.data(); b.inten = inten.data();
    b.bbox_w = bw.data(); b.bbox_h = bh.data(); b.min_inten = mn.data(); b.max_inten = mx.data();
    if (have_slide) { b.slide_min = smin.data(); b.slide_max = smax.data(); }
    b.memory = NYXHIP_MEM_HOST;
    const int ncol = nyxhip_n_columns(mask, &s);
    std::vector<double> table(n * (size_t)ncol);
    nyxhip_ctx* ctx = context();
    if (nyxhip_featurize_batch_at(ctx, &b, ox.data(), oy.data(), mask, &s, table.data(), (size_t)ncol) != NYXHIP_OK)
        throw std::runtime_error(std::string("nyxhip_featurize_batch_at: ") + nyxhip_last_error(ctx));
    // table columns are Feature2D order with angle / index expansion (output_2_buffer.cpp:303-584)
    const int na = s.glcm_n_angles;
    for (size_t i = 0; i < n; i++) {
        LR& r = (*roiData)[(*labels)[start + i]];
        const double* p = table.data() + i * (size_t)ncol;
        auto put = [&](Feature2D first, Feature2D last, int width) {
            for (int f = (int)first; f <= (int)last; f++) { r.fvals[f].assign(p, p + width); p += width; }
        };
        if (mask & NYXHIP_FAM_INTENSITY) put(Feature2D::COV, Feature2D::UNIFORMITY_PIU, 1);
        if (mask & NYXHIP_FAM_ELLIPSE) put(Feature2D::MAJOR_AXIS_LENGTH, Feature2D::ROUNDNESS, 1);
        if (mask & NYXHIP_FAM_EROSION) put(Feature2D::EROSIONS_2_VANISH, Feature2D::EROSIONS_2_VANISH_COMPLEMENT, 1);
        if (mask & NYXHIP_FAM_FRACTAL) put(Feature2D::FRACT_DIM_BOXCOUNT, Feature2D::FRACT_DIM_PERIMETER, 1);
        if (mask & NYXHIP_FAM_FERET) put(Feature2D::MIN_FERET_ANGLE, Feature2D::STAT_FERET_DIAM_MODE, 1);
        if (mask & NYXHIP_FAM_MARTIN) put(Feature2D::STAT_MARTIN_DIAM_MIN, Feature2D::STAT_MARTIN_DIAM_MODE, 1);
        if (mask & NYXHIP_FAM_NASSENSTEIN) put(Feature2D::STAT_NASSENSTEIN_DIAM_MIN, Feature2D::STAT_NASSENSTEIN_DIAM_MODE, 1);
        if (mask & NYXHIP_FAM_CHORDS) put(Feature2D::MAXCHORDS_MAX, Feature2D::ALLCHORDS_STDDEV, 1);
        if (mask & NYXHIP_FAM_EULER) put(Feature2D::EULER_NUMBER, Feature2D::EULER_NUMBER, 1);
        if (mask & NYXHIP_FAM_CIRCLES) put(Feature2D::DIAMETER_MIN_ENCLOSING_CIRCLE, Feature2D::DIAMETER_INSCRIBING_CIRCLE, 1);
        if (mask & NYXHIP_FAM_GEODETIC) put(Feature2D::GEODETIC_LENGTH, Feature2D::THICKNESS, 1);
        if (mask & NYXHIP_FAM_ROI_RADIUS) put(Feature2D::ROI_RADIUS_MEAN, Feature2D::ROI_RADIUS_MEDIAN, 1);
        if (mask & NYXHIP_FAM_GLCM) { put(Feature2D::GLCM_ASM, Feature2D::GLCM_VARIANCE, na); put(Feature2D::GLCM_ASM_AVE, Feature2D::GLCM_SUMVARIANCE_AVE, 1); }
        if (mask & NYXHIP_FAM_GLRLM) { put(Feature2D::GLRLM_SRE, Feature2D::GLRLM_LRHGLE, 4); put(Feature2D::GLRLM_SRE_AVE, Feature2D::GLRLM_LRHGLE_AVE, 1); }
        if (mask & NYXHIP_FAM_GLDZM) put(Feature2D::GLDZM_SDE, Feature2D::GLDZM_ZDE, 1);
        if (mask & NYXHIP_FAM_GLSZM) put(Feature2D::GLSZM_SAE, Feature2D::GLSZM_LAHGLE, 1);
        if (mask & NYXHIP_FAM_GLDM) put(Feature2D::GLDM_SDE, Feature2D::GLDM_LDHGLE, 1);
        if (mask & NYXHIP_FAM_NGLDM) put(Feature2D::NGLDM_LDE, Feature2D::NGLDM_DCENE, 1);
        if (mask & NYXHIP_FAM_NGTDM) put(Feature2D::NGTDM_COARSENESS, Feature2D::NGTDM_STRENGTH, 1);
        if (mask & NYXHIP_FAM_RADIAL) put(Feature2D::FRAC_AT_D, Feature2D::FRAC_AT_D, 8);
        if (mask & NYXHIP_FAM_GABOR) put(Feature2D::GABOR, Feature2D::GABOR, s.gabor_n_filters);
        if (mask & NYXHIP_FAM_RADIAL) put(Feature2D::MEAN_FRAC, Feature2D::RADIAL_CV, 8);
        if (mask & NYXHIP_FAM_ZERNIKE) put(Feature2D::ZERNIKE2D, Feature2D::ZERNIKE2D, 30);
        if (mask & NYXHIP_FAM_SMOMS) put(Feature2D::SPAT_MOMENT_00, Feature2D::WEIGHTED_HU_M7, 1);
        if (mask & NYXHIP_FAM_IMOMS) put(Feature2D::IMOM_RM_00, Feature2D::IMOM_WHU7, 1);
    }
}

// ---- FeatureMethod (feature_method.h:11-80) ------------------------------------------------------------
class FeatureMethod {
public:
    std::string feature_info;
    explicit FeatureMethod(const std::string& info) : feature_info(info) {}
    virtual ~FeatureMethod() {}
    virtual void calculate(LR& roi, const Fsettings& settings) = 0;
    virtual void save_value(std::vector<std::vector<double>>& feature_vals) = 0;
    virtual void osized_add_online_pixel(size_t, size_t, uint32_t) { throw std::runtime_error(feature_info + ": out-of-core ROIs are outside the MI355X hot path"); }
    virtual void osized_calculate(LR&, const Fsettings&) { throw std::runtime_error(feature_info + ": out-of-core ROIs are outside the MI355X hot path"); }
    void provide_features(Feature2D first, Feature2D last) { for (int f = (int)first; f <= (int)last; f++) provided.push_back(f); }
    bool provides(int code) const { return std::find(provided.begin(), provided.end(), code) != provided.end(); }
protected:
    std::vector<int> provided;
    std::vector<std::vector<double>> held;   // values of the last calculate(), indexed by Feature2D
    void run_single(uint32_t mask, LR& r, const Fsettings& s, const Dataset& ds)
    {
        std::vector<int> L{r.label};
        std::unordered_map<int, LR> data;
        data[r.label] = r;
        reduce_range(mask, 0, 1, &L, &data, s, ds);
        held = data[r.label].fvals;
    }
    void save_range(std::vector<std::vector<double>>& fv, Feature2D a, Feature2D b) const
    {
        if (fv.size() < (size_t)Feature2D::_COUNT_) fv.resize((size_t)Feature2D::_COUNT_, std::vector<double>(1, 0.0));
        if (held.empty()) throw std::runtime_error(feature_info + ": save_value() before calculate()");
        for (int f = (int)a; f <= (int)b; f++) fv[f] = held[f];
    }
};

#define NYXHIP_FAMILY_CLASS(NAME, MASK, FIRST, LAST)                                                                          \
    class NAME : public FeatureMethod {                                                                                          \
    public:                                                                                                                      \
        NAME() : FeatureMethod(#NAME) { provide_features(Feature2D::FIRST, Feature2D::LAST); }                                   \
        static bool required(const FeatureSet& fs) { return fs.anyEnabledInRange(Feature2D::FIRST, Feature2D::LAST); }            \
        void calculate(LR& r, const Fsettings& s) override { run_single(MASK, r, s, Dataset()); }                                 \
        void calculate(LR& r, const Fsettings& s, const Dataset& ds) { run_single(MASK, r, s, ds); }                              \
        void save_value(std::vector<std::vector<double>>& fv) override { save_range(fv, Feature2D::FIRST, Feature2D::LAST); }     \
        static void extract(LR& r, const Fsettings& s, const Dataset& ds = Dataset()) { NAME f; f.calculate(r, s, ds); f.save_value(r.fvals); } \
        /* the `functype` of parallel.h:13 */                                                                                    \
        static void reduce(size_t start, size_t end, std::vector<int>* labels, std::unordered_map<int, LR>* roiData,              \
                           const Fsettings& s, const Dataset& ds) { reduce_range(MASK, start, end, labels, roiData, s, ds); }     \
        static void parallel_process_1_batch(size_t start, size_t end, std::vector<int>* labels, std::unordered_map<int, LR>* roiData, \
                                             const Fsettings& s, const Dataset& ds) { reduce_range(MASK, start, end, labels, roiData, s, ds); } \
    };

NYXHIP_FAMILY_CLASS(PixelIntensityFeatures, NYXHIP_FAM_INTENSITY, COV, UNIFORMITY_PIU)
NYXHIP_FAMILY_CLASS(GLCMFeature, NYXHIP_FAM_GLCM, GLCM_ASM, GLCM_SUMVARIANCE_AVE)
NYXHIP_FAMILY_CLASS(GLRLMFeature, NYXHIP_FAM_GLRLM, GLRLM_SRE, GLRLM_LRHGLE_AVE)
NYXHIP_FAMILY_CLASS(GLDZMFeature, NYXHIP_FAM_GLDZM, GLDZM_SDE, GLDZM_ZDE)
NYXHIP_FAMILY_CLASS(GLSZMFeature, NYXHIP_FAM_GLSZM, GLSZM_SAE, GLSZM_LAHGLE)
NYXHIP_FAMILY_CLASS(GLDMFeature, NYXHIP_FAM_GLDM, GLDM_SDE, GLDM_LDHGLE)
NYXHIP_FAMILY_CLASS(NGLDMfeature, NYXHIP_FAM_NGLDM, NGLDM_LDE, NGLDM_DCENE)
NYXHIP_FAMILY_CLASS(NGTDMFeature, NYXHIP_FAM_NGTDM, NGTDM_COARSENESS, NGTDM_STRENGTH)
NYXHIP_FAMILY_CLASS(GaborFeature, NYXHIP_FAM_GABOR, GABOR, GABOR)
NYXHIP_FAMILY_CLASS(ZernikeFeature, NYXHIP_FAM_ZERNIKE, ZERNIKE2D, ZERNIKE2D)
// the contour the weighted moments depend on (ContourFeature::reduce, reduce_trivial_rois.cpp:98-111) is built inside the call
NYXHIP_FAMILY_CLASS(Smoms2D_feature, NYXHIP_FAM_SMOMS, SPAT_MOMENT_00, WEIGHTED_HU_M7)
NYXHIP_FAMILY_CLASS(Imoms2D_feature, NYXHIP_FAM_IMOMS, IMOM_RM_00, IMOM_WHU7)
// features/fractal_dim.h, euler_number.h (mode 8), roi_radius.h: the contour the first and the last depend on is built inside the call
NYXHIP_FAMILY_CLASS(FractalDimensionFeature, NYXHIP_FAM_FRACTAL, FRACT_DIM_BOXCOUNT, FRACT_DIM_PERIMETER)
NYXHIP_FAMILY_CLASS(EulerNumberFeature, NYXHIP_FAM_EULER, EULER_NUMBER, EULER_NUMBER)
NYXHIP_FAMILY_CLASS(RoiRadiusFeature, NYXHIP_FAM_ROI_RADIUS, ROI_RADIUS_MEAN, ROI_RADIUS_MEDIAN)
// features/caliper.h: the convex hull they depend on is built inside the call; they read LR::aabb's origin
NYXHIP_FAMILY_CLASS(CaliperFeretFeature, NYXHIP_FAM_FERET, MIN_FERET_ANGLE, STAT_FERET_DIAM_MODE)
NYXHIP_FAMILY_CLASS(CaliperMartinFeature, NYXHIP_FAM_MARTIN, STAT_MARTIN_DIAM_MIN, STAT_MARTIN_DIAM_MODE)
NYXHIP_FAMILY_CLASS(CaliperNassensteinFeature, NYXHIP_FAM_NASSENSTEIN, STAT_NASSENSTEIN_DIAM_MIN, STAT_NASSENSTEIN_DIAM_MODE)
// features/chords.h: reads LR::aabb's origin and the cloud in LR::raw_pixels order
NYXHIP_FAMILY_CLASS(ChordsFeature, NYXHIP_FAM_CHORDS, MAXCHORDS_MAX, ALLCHORDS_STDDEV)
// features/ellipse_fitting.h, features/erosion.h: the pixel cloud only; the erosion's skip reads LR::aux_min / aux_max
NYXHIP_FAMILY_CLASS(EllipseFittingFeature, NYXHIP_FAM_ELLIPSE, MAJOR_AXIS_LENGTH, ROUNDNESS)
NYXHIP_FAMILY_CLASS(ErosionPixelsFeature, NYXHIP_FAM_EROSION, EROSIONS_2_VANISH, EROSIONS_2_VANISH_COMPLEMENT)
// features/circle.h, features/geodetic_len_thickness.h: the contour they depend on is built inside the call; the circle class reads
// LR::aabb's origin (absolute contour points), the geodetic class coordinate differences and the pixel count only
NYXHIP_FAMILY_CLASS(EnclosingInscribingCircumscribingCircleFeature, NYXHIP_FAM_CIRCLES, DIAMETER_MIN_ENCLOSING_CIRCLE, DIAMETER_INSCRIBING_CIRCLE)
NYXHIP_FAMILY_CLASS(GeodeticLengthThicknessFeature, NYXHIP_FAM_GEODETIC, GEODETIC_LENGTH, THICKNESS)

// RadialDistributionFeature (features/radial_distribution.h): its three codes are not contiguous in the enum (GABOR sits
// between FRAC_AT_D and MEAN_FRAC), so the class is spelled out.  The contour it depends on is built inside the call.
class RadialDistributionFeature : public FeatureMethod {
public:
    const static int num_bins = 8, num_features_FracAtD = 8, num_features_MeanFrac = 8, num_features_RadialCV = 8;
    RadialDistributionFeature() : FeatureMethod("RadialDistributionFeature")
    {
        provide_features(Feature2D::FRAC_AT_D, Feature2D::FRAC_AT_D);
        provide_features(Feature2D::MEAN_FRAC, Feature2D::RADIAL_CV);
    }
    static bool required(const FeatureSet& fs) { return fs.anyEnabled({Feature2D::FRAC_AT_D, Feature2D::MEAN_FRAC, Feature2D::RADIAL_CV}); }
    void calculate(LR& r, const Fsettings& s) override { run_single(NYXHIP_FAM_RADIAL, r, s, Dataset()); }
    void calculate(LR& r, const Fsettings& s, const Dataset& ds) { run_single(NYXHIP_FAM_RADIAL, r, s, ds); }
    void save_value(std::vector<std::vector<double>>& fv) override
    {
        save_range(fv, Feature2D::FRAC_AT_D, Feature2D::FRAC_AT_D);
        save_range(fv, Feature2D::MEAN_FRAC, Feature2D::RADIAL_CV);
    }
    static void extract(LR& r, const Fsettings& s, const Dataset& ds = Dataset()) { RadialDistributionFeature f; f.calculate(r, s, ds); f.save_value(r.fvals); }
    static void reduce(size_t start, size_t end, std::vector<int>* labels, std::unordered_map<int, LR>* roiData, const Fsettings& s,
                       const Dataset& ds) { reduce_range(NYXHIP_FAM_RADIAL, start, end, labels, roiData, s, ds); }
    static void parallel_process_1_batch(size_t start, size_t end, std::vector<int>* labels, std::unordered_map<int, LR>* roiData,
                                         const Fsettings& s, const Dataset& ds) { reduce_range(NYXHIP_FAM_RADIAL, start, end, labels, roiData, s, ds); }
};

using Roidata = std::unordered_map<int, LR>;
// The ROIs of one image as the host batch of the entries that relate them to each other (nyxhip_neighbors_batch, nyxhip_hexpoly_batch):
// the labels in ascending order (the order the reference sorts them into, neighbors.cpp:149-152), LR::aabb's origin, and every LR's
// fvals sized for every code.
struct ImageRois {
    std::vector<int> L;
    std::vector<uint32_t> lab, bw, bh, mn, mx, ox, oy, inten;
    std::vector<uint64_t> off;
    std::vector<uint16_t> x, y;
    nyxhip_batch b{};
    ImageRois(const char* who, Roidata& roiData, const std::unordered_set<int>& uniqueLabels) : L(uniqueLabels.begin(), uniqueLabels.end())
    {
        std::sort(L.begin(), L.end());
        const size_t n = L.size();
        lab.resize(n); bw.resize(n); bh.resize(n); mn.resize(n); mx.resize(n); ox.resize(n); oy.resize(n);
        off.assign(n + 1, 0);
        for (size_t i = 0; i < n; i++) {
            LR& r = roiData.at(L[i]);
            if (L[i] < 0 || r.aabb.get_xmin() < 0 || r.aabb.get_ymin() < 0) throw std::runtime_error(std::string(who) + ": negative label or origin");
            lab[i] = (uint32_t)L[i]; bw[i] = (uint32_t)r.aabb.get_width(); bh[i] = (uint32_t)r.aabb.get_height();
            mn[i] = r.aux_min; mx[i] = r.aux_max;
            ox[i] = (uint32_t)r.aabb.get_xmin(); oy[i] = (uint32_t)r.aabb.get_ymin();
            for (const Pixel2& p : r.raw_pixels) { x.push_back((uint16_t)(p.x - r.aabb.get_xmin())); y.push_back((uint16_t)(p.y - r.aabb.get_ymin())); inten.push_back(p.inten); }
            off[i + 1] = inten.size();
            if (r.fvals.size() < (size_t)FeatureHexPoly::_COUNT_) r.fvals.resize((size_t)FeatureHexPoly::_COUNT_, std::vector<double>(1, 0.0));
        }
        b.n_roi = n; b.roi_label = lab.data(); b.px_offset = off.data(); b.x = x.data(); b.y = y.data(); b.inten = inten.data();
        b.bbox_w = bw.data(); b.bbox_h = bh.data(); b.min_inten = mn.data(); b.max_inten = mx.data();
        b.memory = NYXHIP_MEM_HOST;
    }
    ImageRois(const ImageRois&) = delete;
    ImageRois& operator=(const ImageRois&) = delete;
};
// NeighborsFeature (features/neighbors.h): no per-ROI class -- calculate() is empty in the reference too (neighbors.cpp:40-41) -- but a
// reduction over the ROIs of one image: manual_reduce(roiData, settings, uniqueLabels) relates them to each other (boxes that overlap at
// PIXELDISTANCE, then exact contour distances).  Served by nyxhip_neighbors_batch over the labels in ascending order (the order the
// reference sorts them into, neighbors.cpp:149-152) with LR::aabb's origin; the contours are built inside the call.
class NeighborsFeature : public FeatureMethod {
public:
    NeighborsFeature() : FeatureMethod("NeighborsFeature") { provide_features(Feature2D::NUM_NEIGHBORS, Feature2D::ANG_BW_NEIGHBORS_MODE); }
    static bool required(const FeatureSet& fs) { return fs.anyEnabledInRange(Feature2D::NUM_NEIGHBORS, Feature2D::ANG_BW_NEIGHBORS_MODE); }
    void calculate(LR&, const Fsettings&) override {}
    void save_value(std::vector<std::vector<double>>&) override {}
    static void manual_reduce(Roidata& roiData, const Fsettings& fst, const std::unordered_set<int>& uniqueLabels)
    {
        if (uniqueLabels.empty()) return;
        nyxhip_settings s = make_settings(fst);
        const int radius = NYXHIP_STNGS_MISSING(fst) ? 5 : fst[(int)NyxSetting::PIXELDISTANCE].ival;   // (the reference's default neighbor distance)
        ImageRois im("NeighborsFeature", roiData, uniqueLabels);
        const std::vector<int>& L = im.L;
        const size_t n = L.size();
        std::vector<double> table(n * (size_t)NYXHIP_NEIGHBOR_COLS);
        nyxhip_ctx* ctx = context();
        if (nyxhip_neighbors_batch(ctx, &im.b, im.ox.data(), im.oy.data(), nullptr, 0, radius, &s, table.data(), (size_t)NYXHIP_NEIGHBOR_COLS) != NYXHIP_OK)
            throw std::runtime_error(std::string("nyxhip_neighbors_batch: ") + nyxhip_last_error(ctx));
        for (size_t i = 0; i < n; i++) {
            LR& r = roiData.at(L[i]);
            for (int c = 0; c < NYXHIP_NEIGHBOR_COLS; c++)
                r.fvals[(int)Feature2D::NUM_NEIGHBORS + c].assign(1, table[i * (size_t)NYXHIP_NEIGHBOR_COLS + (size_t)c]);
        }
    }
};

// HexagonalityPolygonalityFeature (features/hexagonality_polygonality.h): a closing formula over NUM_NEIGHBORS, PERIMETER, CONVEX_HULL_AREA
// and the Feret diameters of every ROI, so like NeighborsFeature a reduction over the ROIs of one image -- the reference runs it behind the
// classes it depends on; here nyxhip_hexpoly_batch forms all six inputs itself (one contour chain) and closes them, over the labels in
// ascending order with LR::aabb's origin at PIXELDISTANCE.  Rows the class gates hold its `novalue`, -1.
class HexagonalityPolygonalityFeature : public FeatureMethod {
public:
    static constexpr int novalue = -1;
    HexagonalityPolygonalityFeature() : FeatureMethod("HexagonalityPolygonalityFeature")
    {
        for (int f = (int)FeatureHexPoly::_FIRST_; f < (int)FeatureHexPoly::_COUNT_; f++) provided.push_back(f);
    }
    static bool required(const FeatureSet& fs)
    {
        return fs.anyEnabled({FeatureHexPoly::POLYGONALITY_AVE, FeatureHexPoly::HEXAGONALITY_AVE, FeatureHexPoly::HEXAGONALITY_STDDEV});
    }
    void calculate(LR&, const Fsettings&) override {}
    void save_value(std::vector<std::vector<double>>&) override {}
    static void manual_reduce(Roidata& roiData, const Fsettings& fst, const std::unordered_set<int>& uniqueLabels)
    {
        if (uniqueLabels.empty()) return;
        nyxhip_settings s = make_settings(fst);
        const int radius = NYXHIP_STNGS_MISSING(fst) ? 5 : fst[(int)NyxSetting::PIXELDISTANCE].ival;   // (the reference's default neighbor distance)
        ImageRois im("HexagonalityPolygonalityFeature", roiData, uniqueLabels);
        const std::vector<int>& L = im.L;
        const size_t n = L.size();
        std::vector<double> table(n * (size_t)NYXHIP_HEXPOLY_COLS);
        nyxhip_ctx* ctx = context();
        if (nyxhip_hexpoly_batch(ctx, &im.b, im.ox.data(), im.oy.data(), nullptr, 0, radius, &s, table.data(), (size_t)NYXHIP_HEXPOLY_COLS) != NYXHIP_OK)
            throw std::runtime_error(std::string("nyxhip_hexpoly_batch: ") + nyxhip_last_error(ctx));
        for (size_t i = 0; i < n; i++) {
            LR& r = roiData.at(L[i]);
            for (int c = 0; c < NYXHIP_HEXPOLY_COLS; c++)
                r.fvals[(int)FeatureHexPoly::_FIRST_ + c].assign(1, table[i * (size_t)NYXHIP_HEXPOLY_COLS + (size_t)c]);
        }
    }
};

// IntensityHistogramFeatures (features/intensity_histogram.h): a per-ROI class like the family classes above, but without a bit of the family
// mask -- served by nyxhip_ih_batch, which reads the intensities and LR::aux_min / aux_max only.  The class gates itself (IBSI off, fewer
// than 2 bins, a single intensity: 46 times SOFTNAN, intensity_histogram.cpp:304-320), so reduce() may be called under any settings.
// Integer images: the reference's float / HU domain map is the identity here.
class IntensityHistogramFeatures : public FeatureMethod {
public:
    IntensityHistogramFeatures() : FeatureMethod("IntensityHistogramFeatures") { provide_features(Feature2D::IH_MEAN_VAL, Feature2D::IH_BIN_SIZE); }
    static bool required(const FeatureSet& fs) { return fs.anyEnabledInRange(Feature2D::IH_MEAN_VAL, Feature2D::IH_BIN_SIZE); }
    void calculate(LR& r, const Fsettings& s) override { calculate(r, s, Dataset()); }
    void calculate(LR& r, const Fsettings& s, const Dataset& ds)
    {
        std::vector<int> L{r.label};
        std::unordered_map<int, LR> data;
        data[r.label] = r;
        reduce(0, 1, &L, &data, s, ds);
        held = data[r.label].fvals;
    }
    void save_value(std::vector<std::vector<double>>& fv) override { save_range(fv, Feature2D::IH_MEAN_VAL, Feature2D::IH_BIN_SIZE); }
    static void extract(LR& r, const Fsettings& s, const Dataset& ds = Dataset()) { IntensityHistogramFeatures f; f.calculate(r, s, ds); f.save_value(r.fvals); }
    static void reduce(size_t start, size_t end, std::vector<int>* labels, std::unordered_map<int, LR>* roiData, const Fsettings& fst, const Dataset&)
    {
        if (end <= start) return;
        nyxhip_settings s = make_settings(fst);
        const size_t n = end - start;
        std::vector<uint32_t> mn(n), mx(n), inten;
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; i++) {
            LR& r = (*roiData)[(*labels)[start + i]];
            mn[i] = r.aux_min; mx[i] = r.aux_max;
            for (const Pixel2& p : r.raw_pixels) inten.push_back(p.inten);
            off[i + 1] = inten.size();
            if (r.fvals.empty()) r.initialize_fvals();
        }
        nyxhip_batch b{};
        b.n_roi = n; b.px_offset = off.data(); b.inten = inten.data(); b.min_inten = mn.data(); b.max_inten = mx.data();
        b.memory = NYXHIP_MEM_HOST;
        std::vector<double> table(n * (size_t)NYXHIP_IH_COLS);
        nyxhip_ctx* ctx = context();
        if (nyxhip_ih_batch(ctx, &b, &s, table.data(), (size_t)NYXHIP_IH_COLS) != NYXHIP_OK)
            throw std::runtime_error(std::string("nyxhip_ih_batch: ") + nyxhip_last_error(ctx));
        for (size_t i = 0; i < n; i++) {
            LR& r = (*roiData)[(*labels)[start + i]];
            for (int c = 0; c < NYXHIP_IH_COLS; c++)
                r.fvals[(int)Feature2D::IH_MEAN_VAL + c].assign(1, table[i * (size_t)NYXHIP_IH_COLS + (size_t)c]);
        }
    }
};

// FocusScoreFeature (features/focus_score.h) and SaturationFeature (features/saturation.h): the two image-quality classes, over
// nyxhip_imq_batch, which reads the pixel cloud, the box and LR::aux_min / aux_max.  One batch call yields the four columns; each class
// keeps its own two.  A box with a side of 1 has SOFTNAN as LOCAL_FOCUS_SCORE (the reference's loop does not end on it).
inline std::vector<double> imq_batch_table(size_t start, size_t end, std::vector<int>* labels, std::unordered_map<int, LR>* roiData, const Fsettings& fst)
{
    nyxhip_settings s = make_settings(fst);
    const size_t n = end - start;
    std::vector<uint32_t> bw(n), bh(n), mn(n), mx(n), inten;
    std::vector<uint16_t> x, y;
    std::vector<uint64_t> off(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        LR& r = (*roiData)[(*labels)[start + i]];
        bw[i] = r.raw_pixels.empty() ? 0u : (uint32_t)r.aabb.get_width(); bh[i] = r.raw_pixels.empty() ? 0u : (uint32_t)r.aabb.get_height();
        mn[i] = r.aux_min; mx[i] = r.aux_max;
        for (const Pixel2& p : r.raw_pixels) { x.push_back((uint16_t)(p.x - r.aabb.get_xmin())); y.push_back((uint16_t)(p.y - r.aabb.get_ymin())); inten.push_back(p.inten); }
        off[i + 1] = inten.size();
        if (r.fvals.size() < (size_t)FeatureIMQ::_COUNT_) r.fvals.resize((size_t)FeatureIMQ::_COUNT_, std::vector<double>(1, 0.0));
    }
    nyxhip_batch b{};
    b.n_roi = n; b.px_offset = off.data(); b.x = x.data(); b.y = y.data(); b.inten = inten.data();
    b.bbox_w = bw.data(); b.bbox_h = bh.data(); b.min_inten = mn.data(); b.max_inten = mx.data();
    b.memory = NYXHIP_MEM_HOST;
    std::vector<double> table(n * (size_t)NYXHIP_IMQ_COLS);
    nyxhip_ctx* ctx = context();
    if (nyxhip_imq_batch(ctx, &b, &s, table.data(), (size_t)NYXHIP_IMQ_COLS) != NYXHIP_OK)
        throw std::runtime_error(std::string("nyxhip_imq_batch: ") + nyxhip_last_error(ctx));
    return table;
}

// CLASS: the class name; A, B: its two codes; CA, CB: their columns in the table of nyxhip_imq_batch
#define NYXHIP_IMQ_CLASS(CLASS, A, B, CA, CB)                                                                                                  \
    class CLASS : public FeatureMethod {                                                                                                      \
    public:                                                                                                                                   \
        CLASS() : FeatureMethod(#CLASS) { provided.push_back((int)FeatureIMQ::A); provided.push_back((int)FeatureIMQ::B); }                   \
        static bool required(const FeatureSet& fs) { return fs.anyEnabled({FeatureIMQ::A, FeatureIMQ::B}); }                                  \
        void calculate(LR& r, const Fsettings& s) override                                                                                    \
        {                                                                                                                                     \
            std::vector<int> L{r.label};                                                                                                      \
            std::unordered_map<int, LR> data;                                                                                                 \
            data[r.label] = r;                                                                                                                \
            reduce(0, 1, &L, &data, s, Dataset());                                                                                            \
            held = data[r.label].fvals;                                                                                                       \
        }                                                                                                                                     \
        void save_value(std::vector<std::vector<double>>& fv) override                                                                        \
        {                                                                                                                                     \
            if (held.empty()) throw std::runtime_error(feature_info + ": save_value() before calculate()");                                   \
            if (fv.size() < (size_t)FeatureIMQ::_COUNT_) fv.resize((size_t)FeatureIMQ::_COUNT_, std::vector<double>(1, 0.0));                 \
            fv[(int)FeatureIMQ::A] = held[(int)FeatureIMQ::A]; fv[(int)FeatureIMQ::B] = held[(int)FeatureIMQ::B];                             \
        }                                                                                                                                     \
        static void extract(LR& r, const Fsettings& s) { CLASS f; f.calculate(r, s); f.save_value(r.fvals); }                                 \
        static void reduce(size_t start, size_t end, std::vector<int>* labels, std::unordered_map<int, LR>* roiData, const Fsettings& fst,    \
                           const Dataset&)                                                                                                    \
        {                                                                                                                                     \
            if (end <= start) return;                                                                                                         \
            const std::vector<double> table = imq_batch_table(start, end, labels, roiData, fst);                                              \
            for (size_t i = 0; i < end - start; i++) {                                                                                        \
                LR& r = (*roiData)[(*labels)[start + i]];                                                                                     \
                r.fvals[(int)FeatureIMQ::A].assign(1, table[i * (size_t)NYXHIP_IMQ_COLS + CA]);                                               \
                r.fvals[(int)FeatureIMQ::B].assign(1, table[i * (size_t)NYXHIP_IMQ_COLS + CB]);                                               \
            }                                                                                                                                 \
        }                                                                                                                                     \
        static void parallel_process_1_batch(size_t start, size_t end, std::vector<int>* labels, std::unordered_map<int, LR>* roiData,        \
                                             const Fsettings& fst, const Dataset& ds) { reduce(start, end, labels, roiData, fst, ds); }       \
    };
NYXHIP_IMQ_CLASS(FocusScoreFeature, FOCUS_SCORE, LOCAL_FOCUS_SCORE, 0, 1)
NYXHIP_IMQ_CLASS(SaturationFeature, MAX_SATURATION, MIN_SATURATION, 2, 3)
#undef NYXHIP_IMQ_CLASS

// runParallel (parallel.h:23-42): the GPU batch is the parallel unit, so the slices run back to back on the
// caller's thread -- same observable contract (every label of [0, datasetSize) reduced on return).
typedef void (*functype)(size_t, size_t, std::vector<int>*, std::unordered_map<int, LR>*, const Fsettings&, const Dataset&);
inline void runParallel(functype f, int /*nThr*/, size_t /*workPerThread*/, size_t datasetSize, std::vector<int>* labels,
                        std::unordered_map<int, LR>* roiData, const Fsettings& s, const Dataset& ds)
{
    f(0, datasetSize, labels, roiData, s, ds);
}

// reduce_trivial_rois_manual (reduce_trivial_rois.cpp:772-795): every required family in ONE fused batch call.
inline void reduce_trivial_rois_manual(std::vector<int>& PendingRoisLabels, std::unordered_map<int, LR>& roiData, const FeatureSet& fs,
                                       const Fsettings& s, const Dataset& ds)
{
    uint32_t mask = 0;
    if (PixelIntensityFeatures::required(fs)) mask |= NYXHIP_FAM_INTENSITY;
    if (FractalDimensionFeature::required(fs)) mask |= NYXHIP_FAM_FRACTAL;
    if (CaliperFeretFeature::required(fs)) mask |= NYXHIP_FAM_FERET;
    if (CaliperMartinFeature::required(fs)) mask |= NYXHIP_FAM_MARTIN;
    if (CaliperNassensteinFeature::required(fs)) mask |= NYXHIP_FAM_NASSENSTEIN;
    if (ChordsFeature::required(fs)) mask |= NYXHIP_FAM_CHORDS;
    if (EllipseFittingFeature::required(fs)) mask |= NYXHIP_FAM_ELLIPSE;
    if (ErosionPixelsFeature::required(fs)) mask |= NYXHIP_FAM_EROSION;
    if (EulerNumberFeature::required(fs)) mask |= NYXHIP_FAM_EULER;
    if (EnclosingInscribingCircumscribingCircleFeature::required(fs)) mask |= NYXHIP_FAM_CIRCLES;
    if (GeodeticLengthThicknessFeature::required(fs)) mask |= NYXHIP_FAM_GEODETIC;
    if (RoiRadiusFeature::required(fs)) mask |= NYXHIP_FAM_ROI_RADIUS;
    if (GLCMFeature::required(fs)) mask |= NYXHIP_FAM_GLCM;
    if (GLRLMFeature::required(fs)) mask |= NYXHIP_FAM_GLRLM;
    if (GLDZMFeature::required(fs)) mask |= NYXHIP_FAM_GLDZM;   // reduce_trivial_rois.cpp:215-220
    if (GLSZMFeature::required(fs)) mask |= NYXHIP_FAM_GLSZM;
    if (GLDMFeature::required(fs)) mask |= NYXHIP_FAM_GLDM;     // :231-236
    if (NGLDMfeature::required(fs)) mask |= NYXHIP_FAM_NGLDM;   // :239-244
    if (NGTDMFeature::required(fs)) mask |= NYXHIP_FAM_NGTDM;
    if (GaborFeature::required(fs)) mask |= NYXHIP_FAM_GABOR;
    if (RadialDistributionFeature::required(fs)) mask |= NYXHIP_FAM_RADIAL;   // reduce_trivial_rois.cpp (RadialDistributionFeature)
    if (ZernikeFeature::required(fs)) mask |= NYXHIP_FAM_ZERNIKE;
    if (Smoms2D_feature::required(fs)) mask |= NYXHIP_FAM_SMOMS;   // reduce_trivial_rois.cpp:326-331
    if (Imoms2D_feature::required(fs)) mask |= NYXHIP_FAM_IMOMS;   // :320-325
    if (mask) reduce_range(mask, 0, PendingRoisLabels.size(), &PendingRoisLabels, &roiData, s, ds);
    if (IntensityHistogramFeatures::required(fs))                  // a call of its own: the class has no bit of the family mask
        IntensityHistogramFeatures::reduce(0, PendingRoisLabels.size(), &PendingRoisLabels, &roiData, s, ds);
    if (FocusScoreFeature::required(fs))                           // reduce_trivial_rois.cpp:388-393
        FocusScoreFeature::reduce(0, PendingRoisLabels.size(), &PendingRoisLabels, &roiData, s, ds);
    if (SaturationFeature::required(fs))                           // :401-405
        SaturationFeature::reduce(0, PendingRoisLabels.size(), &PendingRoisLabels, &roiData, s, ds);
}

} // namespace NyxusHip
