// nyxhip_columns.hip -- the column catalogue of include/nyxhip.h (host only): names, counts, settings checks, defaults.
#include "nyxhip_ctx.h"

using namespace nyxhip;

namespace {

// ---- column catalogue (Feature2D enum order; names = user-facing feature names,
// src/nyx/featureset.cpp UserFacingFeatureNames) -------------------------------------
const char* kIntensityNames[kIntensityCols] = {
    "COV", "COVERED_IMAGE_INTENSITY_RANGE", "ENERGY", "ENTROPY", "EXCESS_KURTOSIS", "HYPERFLATNESS",
    "HYPERSKEWNESS", "INTEGRATED_INTENSITY", "INTERQUARTILE_RANGE", "KURTOSIS", "MAX", "MEAN",
    "MEAN_ABSOLUTE_DEVIATION", "MEDIAN", "MEDIAN_ABSOLUTE_DEVIATION", "MIN", "MODE", "P01", "P10", "P25",
    "P75", "P90", "P99", "QCOD", "RANGE", "ROBUST_MEAN", "ROBUST_MEAN_ABSOLUTE_DEVIATION",
    "ROOT_MEAN_SQUARED", "SKEWNESS", "STANDARD_DEVIATION", "STANDARD_DEVIATION_BIASED", "STANDARD_ERROR",
    "VARIANCE", "VARIANCE_BIASED", "UNIFORMITY", "UNIFORMITY_PIU"};
const char* kGlcmNames[kGlcmAngled] = {
    "GLCM_ASM", "GLCM_ACOR", "GLCM_CLUPROM", "GLCM_CLUSHADE", "GLCM_CLUTEND", "GLCM_CONTRAST",
    "GLCM_CORRELATION", "GLCM_DIFAVE", "GLCM_DIFENTRO", "GLCM_DIFVAR", "GLCM_DIS", "GLCM_ENERGY",
    "GLCM_ENTROPY", "GLCM_HOM1", "GLCM_HOM2", "GLCM_ID", "GLCM_IDN", "GLCM_IDM", "GLCM_IDMN",
    "GLCM_INFOMEAS1", "GLCM_INFOMEAS2", "GLCM_IV", "GLCM_JAVE", "GLCM_JE", "GLCM_JMAX", "GLCM_JVAR",
    "GLCM_SUMAVERAGE", "GLCM_SUMENTROPY", "GLCM_SUMVARIANCE", "GLCM_VARIANCE"};
const char* kGlcmAveNames[kGlcmAve] = {
    "GLCM_ASM_AVE", "GLCM_ACOR_AVE", "GLCM_CLUPROM_AVE", "GLCM_CLUSHADE_AVE", "GLCM_CLUTEND_AVE",
    "GLCM_CONTRAST_AVE", "GLCM_CORRELATION_AVE", "GLCM_DIFAVE_AVE", "GLCM_DIFENTRO_AVE", "GLCM_DIFVAR_AVE",
    "GLCM_DIS_AVE", "GLCM_ENERGY_AVE", "GLCM_ENTROPY_AVE", "GLCM_HOM1_AVE", "GLCM_ID_AVE", "GLCM_IDN_AVE",
    "GLCM_IDM_AVE", "GLCM_IDMN_AVE", "GLCM_IV_AVE", "GLCM_JAVE_AVE", "GLCM_JE_AVE", "GLCM_INFOMEAS1_AVE",
    "GLCM_INFOMEAS2_AVE", "GLCM_VARIANCE_AVE", "GLCM_JMAX_AVE", "GLCM_JVAR_AVE", "GLCM_SUMAVERAGE_AVE",
    "GLCM_SUMENTROPY_AVE", "GLCM_SUMVARIANCE_AVE"};

const char* kGlrlmNames[16] = {"GLRLM_SRE", "GLRLM_LRE", "GLRLM_GLN", "GLRLM_GLNN", "GLRLM_RLN", "GLRLM_RLNN", "GLRLM_RP",
                               "GLRLM_GLV", "GLRLM_RV", "GLRLM_RE", "GLRLM_LGLRE", "GLRLM_HGLRE", "GLRLM_SRLGLE",
                               "GLRLM_SRHGLE", "GLRLM_LRLGLE", "GLRLM_LRHGLE"};
const char* kGlszmNames[16] = {"GLSZM_SAE", "GLSZM_LAE", "GLSZM_GLN", "GLSZM_GLNN", "GLSZM_SZN", "GLSZM_SZNN", "GLSZM_ZP",
                               "GLSZM_GLV", "GLSZM_ZV", "GLSZM_ZE", "GLSZM_LGLZE", "GLSZM_HGLZE", "GLSZM_SALGLE",
                               "GLSZM_SAHGLE", "GLSZM_LALGLE", "GLSZM_LAHGLE"};
const char* kGldzmNames[18] = {"GLDZM_SDE", "GLDZM_LDE", "GLDZM_LGLZE", "GLDZM_HGLZE", "GLDZM_SDLGLE", "GLDZM_SDHGLE", "GLDZM_LDLGLE",
                               "GLDZM_LDHGLE", "GLDZM_GLNU", "GLDZM_GLNUN", "GLDZM_ZDNU", "GLDZM_ZDNUN", "GLDZM_ZP", "GLDZM_GLM",
                               "GLDZM_GLV", "GLDZM_ZDM", "GLDZM_ZDV", "GLDZM_ZDE"};
const char* kGldmNames[14] = {"GLDM_SDE", "GLDM_LDE", "GLDM_GLN", "GLDM_DN", "GLDM_DNN", "GLDM_GLV", "GLDM_DV", "GLDM_DE", "GLDM_LGLE",
                              "GLDM_HGLE", "GLDM_SDLGLE", "GLDM_SDHGLE", "GLDM_LDLGLE", "GLDM_LDHGLE"};
const char* kNgldmNames[19] = {"NGLDM_LDE", "NGLDM_HDE", "NGLDM_LGLCE", "NGLDM_HGLCE", "NGLDM_LDLGLE", "NGLDM_LDHGLE", "NGLDM_HDLGLE",
                               "NGLDM_HDHGLE", "NGLDM_GLNU", "NGLDM_GLNUN", "NGLDM_DCNU", "NGLDM_DCNUN", "NGLDM_DCP", "NGLDM_GLM",
                               "NGLDM_GLV", "NGLDM_DCM", "NGLDM_DCV", "NGLDM_DCENT", "NGLDM_DCENE"};
const char* kNgtdmNames[5] = {"NGTDM_COARSENESS", "NGTDM_CONTRAST", "NGTDM_BUSYNESS", "NGTDM_COMPLEXITY", "NGTDM_STRENGTH"};
const int kGlrlmAngles[4] = {0, 45, 90, 135}; // GLRLMFeature::rotAngles, glrlm.h:134

} // namespace

namespace nyxhip {

bool settings_ok(const nyxhip_settings* s, uint32_t mask, std::string& why)
{
    if (!s) { why = "settings is NULL"; return false; }
    if (mask & NYXHIP_FAM_INTENSITY) {
        if (s->grey_depth == 0) { why = "grey_depth must be non-zero (histogram bin count)"; return false; }
    }
    if (mask & NYXHIP_FAM_GLCM) {
        if (s->glcm_n_angles < 0 || s->glcm_n_angles > NYXHIP_MAX_GLCM_ANGLES) { why = "glcm_n_angles out of range"; return false; }
        for (int i = 0; i < s->glcm_n_angles; i++) {
            int a = s->glcm_angles[i];
            if (a != 0 && a != 45 && a != 90 && a != 135) { why = "unsupported GLCM angle (glcm.cpp:252-254)"; return false; }
        }
        if (s->glcm_offset < 0) { why = "glcm_offset must be >= 0"; return false; }
    }
    if ((mask & NYXHIP_FAM_NGLDM) && !s->ibsi && s->grey_depth < 0) {
        // ngldm.cpp:201 passes GREYDEPTH as unsigned: a negative depth becomes ~4.29e9 levels (one per intensity)
        why = "NGLDM with a negative (radiomics) grey depth is not supported";
        return false;
    }
    if ((mask & NYXHIP_FAM_GLDZM) && !s->ibsi && s->grey_depth < 0) {
        // radiomics binning leaves level-0 background zones: the reference writes them one row past its matrix
        // (gldzm.cpp:44-50) and its distances depend on the flood order (zeros turn VISITED, :111-116) -- undefined there
        why = "GLDZM with a negative (radiomics) grey depth is not supported (undefined in the reference)";
        return false;
    }
    if (mask & NYXHIP_FAM_GABOR) {
        if (s->gabor_n_filters < 0 || s->gabor_n_filters > NYXHIP_MAX_GABOR_FILTERS) { why = "gabor_n_filters out of range"; return false; }
        if (s->gabor_kersize < 1 || s->gabor_kersize > 64) { why = "gabor_kersize out of range (1..64)"; return false; }
    }
    return true;
}

} // namespace nyxhip

namespace {

std::vector<std::string> column_names(uint32_t mask, const nyxhip_settings* s)
{
    std::vector<std::string> v;
    if (mask & NYXHIP_FAM_INTENSITY)
        for (auto n : kIntensityNames) v.push_back(n);
    // the shape block follows the intensity block (featureset.h:46-160)
    if (mask & NYXHIP_FAM_ELLIPSE)    // EllipseFittingFeature (featureset.h:62-68)
        for (auto n : {"MAJOR_AXIS_LENGTH", "MINOR_AXIS_LENGTH", "ELONGATION", "ECCENTRICITY", "ORIENTATION", "ROUNDNESS"}) v.push_back(n);
    if (mask & NYXHIP_FAM_EROSION) { v.push_back("EROSIONS_2_VANISH"); v.push_back("EROSIONS_2_VANISH_COMPLEMENT"); }   // featureset.h:85-86
    if (mask & NYXHIP_FAM_FRACTAL) { v.push_back("FRACT_DIM_BOXCOUNT"); v.push_back("FRACT_DIM_PERIMETER"); }
    {   // the caliper classes (featureset.h:93-114; names: featureset.cpp:181-203)
        const char* st[6] = {"MIN", "MAX", "MEAN", "MEDIAN", "STDDEV", "MODE"};
        if (mask & NYXHIP_FAM_FERET) {
            v.push_back("MIN_FERET_ANGLE"); v.push_back("MAX_FERET_ANGLE");
            for (auto k : st) v.push_back(std::string("STAT_FERET_DIAM_") + k);
        }
        if (mask & NYXHIP_FAM_MARTIN)
            for (auto k : st) v.push_back(std::string("STAT_MARTIN_DIAM_") + k);
        if (mask & NYXHIP_FAM_NASSENSTEIN)
            for (auto k : st) v.push_back(std::string("STAT_NASSENSTEIN_DIAM_") + k);
    }
    if (mask & NYXHIP_FAM_CHORDS) {   // ChordsFeature (featureset.h:117-132; names: featureset.cpp:205-220)
        const char* st[8] = {"MAX", "MAX_ANG", "MIN", "MIN_ANG", "MEDIAN", "MEAN", "MODE", "STDDEV"};
        for (auto g : {"MAXCHORDS_", "ALLCHORDS_"})
            for (auto k : st) v.push_back(std::string(g) + k);
    }
    if (mask & NYXHIP_FAM_EULER) v.push_back("EULER_NUMBER");
    if (mask & NYXHIP_FAM_CIRCLES)    // EnclosingInscribingCircumscribingCircleFeature (featureset.h:150-152)
        for (auto n : {"DIAMETER_MIN_ENCLOSING_CIRCLE", "DIAMETER_CIRCUMSCRIBING_CIRCLE", "DIAMETER_INSCRIBING_CIRCLE"}) v.push_back(n);
    if (mask & NYXHIP_FAM_GEODETIC) { v.push_back("GEODETIC_LENGTH"); v.push_back("THICKNESS"); }   // featureset.h:154-155
    if (mask & NYXHIP_FAM_ROI_RADIUS) { v.push_back("ROI_RADIUS_MEAN"); v.push_back("ROI_RADIUS_MAX"); v.push_back("ROI_RADIUS_MEDIAN"); }
    if (mask & NYXHIP_FAM_GLCM) {
        for (auto n : kGlcmNames)
            for (int a = 0; a < s->glcm_n_angles; a++)
                v.push_back(std::string(n) + "_" + std::to_string(s->glcm_angles[a])); // output_2_buffer.cpp:336-343
        for (auto n : kGlcmAveNames) v.push_back(n);
    }
    if (mask & NYXHIP_FAM_GLRLM) {
        for (auto n : kGlrlmNames)
            for (int a : kGlrlmAngles) v.push_back(std::string(n) + "_" + std::to_string(a)); // output_2_buffer.cpp:351-361
        for (auto n : kGlrlmNames) v.push_back(std::string(n) + "_AVE");
    }
    if (mask & NYXHIP_FAM_GLDZM)
        for (auto n : kGldzmNames) v.push_back(n);
    if (mask & NYXHIP_FAM_GLSZM)
        for (auto n : kGlszmNames) v.push_back(n);
    if (mask & NYXHIP_FAM_GLDM)
        for (auto n : kGldmNames) v.push_back(n);
    if (mask & NYXHIP_FAM_NGLDM)
        for (auto n : kNgldmNames) v.push_back(n);
    if (mask & NYXHIP_FAM_NGTDM)
        for (auto n : kNgtdmNames) v.push_back(n);
    // FRAC_AT_D, GABOR, MEAN_FRAC, RADIAL_CV, ZERNIKE2D: the enum interleaves the radial distribution with Gabor (featureset.h:352-357)
    if (mask & NYXHIP_FAM_RADIAL)
        for (int i = 0; i < kRadialBins; i++) v.push_back("FRAC_AT_D_" + std::to_string(i));          // output_2_buffer.cpp:374-383
    if (mask & NYXHIP_FAM_GABOR)
        for (int i = 0; i < s->gabor_n_filters; i++) v.push_back("GABOR_" + std::to_string(i));       // output_2_buffer.cpp:364-373
    if (mask & NYXHIP_FAM_RADIAL) {
        for (int i = 0; i < kRadialBins; i++) v.push_back("MEAN_FRAC_" + std::to_string(i));          // :385-397
        for (int i = 0; i < kRadialBins; i++) v.push_back("RADIAL_CV_" + std::to_string(i));          // :399-411
    }
    if (mask & NYXHIP_FAM_ZERNIKE)
        for (int i = 0; i < kZernikeCols; i++) v.push_back("ZERNIKE2D_Z" + std::to_string(i));        // :417-427
    if (mask & NYXHIP_FAM_SMOMS) {     // featureset.h:362-467
        const char* pq13[13] = {"00", "01", "02", "03", "10", "11", "12", "13", "20", "21", "22", "23", "30"};
        const char* pq7[7] = {"02", "03", "11", "12", "20", "21", "30"};
        const char* pq10[10] = {"00", "01", "02", "03", "10", "11", "12", "20", "21", "30"};
        for (auto k : pq13) v.push_back(std::string("SPAT_MOMENT_") + k);
        for (int p = 0; p < 4; p++) for (int q = 0; q < 4; q++) v.push_back("CENTRAL_MOMENT_" + std::to_string(p) + std::to_string(q));
        for (int p = 0; p < 4; p++) for (int q = 0; q < 4; q++) v.push_back("NORM_SPAT_MOMENT_" + std::to_string(p) + std::to_string(q));
        for (auto k : pq7) v.push_back(std::string("NORM_CENTRAL_MOMENT_") + k);
        for (int k = 1; k <= 7; k++) v.push_back("HU_M" + std::to_string(k));
        for (auto k : pq10) v.push_back(std::string("WEIGHTED_SPAT_MOMENT_") + k);
        for (auto k : pq7) v.push_back(std::string("WEIGHTED_CENTRAL_MOMENT_") + k);
        for (auto k : pq7) v.push_back(std::string("WT_NORM_CTR_MOM_") + k);
        for (int k = 1; k <= 7; k++) v.push_back("WEIGHTED_HU_M" + std::to_string(k));
    }
    if (mask & NYXHIP_FAM_IMOMS) {     // featureset.h:472-565
        const char* pq13[13] = {"00", "01", "02", "03", "10", "11", "12", "13", "20", "21", "22", "23", "30"};
        const char* pq7[7] = {"02", "03", "11", "12", "20", "21", "30"};
        const char* pq10[10] = {"00", "01", "02", "03", "10", "11", "12", "20", "21", "30"};
        for (auto k : pq13) v.push_back(std::string("IMOM_RM_") + k);
        for (int p = 0; p < 4; p++) for (int q = 0; q < 4; q++) v.push_back("IMOM_CM_" + std::to_string(p) + std::to_string(q));
        for (int p = 0; p < 4; p++) for (int q = 0; q < 4; q++) v.push_back("IMOM_NRM_" + std::to_string(p) + std::to_string(q));
        for (auto k : pq7) v.push_back(std::string("IMOM_NCM_") + k);
        for (int k = 1; k <= 7; k++) v.push_back("IMOM_HU" + std::to_string(k));
        for (auto k : pq10) v.push_back(std::string("IMOM_WRM_") + k);
        for (auto k : pq7) v.push_back(std::string("IMOM_WCM_") + k);
        for (auto k : pq7) v.push_back(std::string("IMOM_WNCM_") + k);
        for (int k = 1; k <= 7; k++) v.push_back("IMOM_WHU" + std::to_string(k));
    }
    return v;
}

} // namespace

extern "C" {

void nyxhip_default_settings(nyxhip_settings* s)
{
    if (!s) return;
    memset(s, 0, sizeof(*s));
    s->soft_nan = 0.0;                 // cli_result_options.h:75
    s->tiny = 1e-10;
    s->grey_depth = 64;                // environment: coarse gray depth default
    s->ibsi = 0;
    s->glcm_grey_depth = 64;
    s->glcm_offset = 1;                // env_features.cpp:727
    s->glcm_n_angles = 4;              // glcm.cpp:9
    s->glcm_angles[0] = 0; s->glcm_angles[1] = 45; s->glcm_angles[2] = 90; s->glcm_angles[3] = 135;
    s->glcm_symmetric = 0;             // glcm.cpp:8
    s->gabor_gamma = 0.1; s->gabor_sig2lam = 0.8; s->gabor_kersize = 16; s->gabor_f0lp = 0.1; s->gabor_graythr = 0.025;
    s->gabor_n_filters = 4;            // gabor.cpp:19-25, consumed as (first = f0, second = theta) at :107-110
    const double pi4 = 0.78539816339744830962;
    const double f0[4] = {0.0, pi4, 2 * pi4, pi4 * 3.0}, th[4] = {4.0, 16.0, 32.0, 64.0};
    for (int i = 0; i < 4; i++) { s->gabor_f0[i] = f0[i]; s->gabor_theta[i] = th[i]; }
}

int nyxhip_n_columns(uint32_t family_mask, const nyxhip_settings* s)
{
    if (!s) return 0;
    int n = 0;
    if (family_mask & NYXHIP_FAM_INTENSITY) n += kIntensityCols;
    if (family_mask & NYXHIP_FAM_ELLIPSE) n += kEllipseCols;
    if (family_mask & NYXHIP_FAM_EROSION) n += kErosionCols;
    if (family_mask & NYXHIP_FAM_FRACTAL) n += kFractalCols;
    if (family_mask & NYXHIP_FAM_FERET) n += kFeretCols;
    if (family_mask & NYXHIP_FAM_MARTIN) n += kMartinCols;
    if (family_mask & NYXHIP_FAM_NASSENSTEIN) n += kNassensteinCols;
    if (family_mask & NYXHIP_FAM_CHORDS) n += kChordsCols;
    if (family_mask & NYXHIP_FAM_EULER) n += kEulerCols;
    if (family_mask & NYXHIP_FAM_CIRCLES) n += kCirclesCols;
    if (family_mask & NYXHIP_FAM_GEODETIC) n += kGeodeticCols;
    if (family_mask & NYXHIP_FAM_ROI_RADIUS) n += kRoiRadiusCols;
    if (family_mask & NYXHIP_FAM_GLCM) n += kGlcmAngled * s->glcm_n_angles + kGlcmAve;
    if (family_mask & NYXHIP_FAM_GLRLM) n += kGlrlmCols;
    if (family_mask & NYXHIP_FAM_GLDZM) n += kGldzmCols;
    if (family_mask & NYXHIP_FAM_GLSZM) n += kGlszmCols;
    if (family_mask & NYXHIP_FAM_GLDM) n += kGldmCols;
    if (family_mask & NYXHIP_FAM_NGLDM) n += kNgldmCols;
    if (family_mask & NYXHIP_FAM_NGTDM) n += kNgtdmCols;
    if (family_mask & NYXHIP_FAM_GABOR) n += s->gabor_n_filters;
    if (family_mask & NYXHIP_FAM_ZERNIKE) n += kZernikeCols;
    if (family_mask & NYXHIP_FAM_SMOMS) n += kMomCols;
    if (family_mask & NYXHIP_FAM_IMOMS) n += kMomCols;
    if (family_mask & NYXHIP_FAM_RADIAL) n += kRadialCols;
    return n;
}

int nyxhip_column_name(uint32_t family_mask, const nyxhip_settings* s, int col, char* buf, size_t buf_len)
{
    if (!s || !buf || buf_len == 0) return NYXHIP_ERR_INVALID_ARG;
    // callers walk a mask's columns one call per column: the list of the last (mask, settings) asked for is kept per thread
    struct Key { uint32_t mask; int32_t na, nf, ang[NYXHIP_MAX_GLCM_ANGLES]; };
    Key key{family_mask & kImplemented, s->glcm_n_angles, s->gabor_n_filters, {}};
    for (int a = 0; a < NYXHIP_MAX_GLCM_ANGLES; a++) key.ang[a] = s->glcm_angles[a];
    thread_local Key last_key;
    thread_local bool have_last = false;
    thread_local std::vector<std::string> last;
    if (!have_last || memcmp(&key, &last_key, sizeof(Key)) != 0) {
        last = column_names(key.mask, s);
        last_key = key;
        have_last = true;
    }
    const auto& v = last;
    if (col < 0 || col >= (int)v.size()) return NYXHIP_ERR_INVALID_ARG;
    snprintf(buf, buf_len, "%s", v[col].c_str());
    return NYXHIP_OK;
}

void nyxhip_finalize_table(double* table, size_t n_rows, size_t n_cols, size_t ld, double soft_nan)
{
    if (!table) return;
    for (size_t r = 0; r < n_rows; r++)
        for (size_t c = 0; c < n_cols; c++) {
            double& v = table[r * ld + c];
            if (isnan(v) || isinf(v)) v = soft_nan; // force_finite_number, helpers/helpers.h:376-382
        }
}

} // extern "C"
