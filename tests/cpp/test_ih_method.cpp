// test_ih_method.cpp -- IntensityHistogramFeatures of include/nyxhip_feature_method.hpp, used the way the reference's workflow uses its
// class: LRs fed pixel by pixel, runParallel(IntensityHistogramFeatures::reduce, ...) under IBSI settings, then the 46 fvals of every ROI
// against the recorded values; calculate() + save_value() on one ROI; the class's own gate with IBSI off.
// Input: a text file "grey_depth soft_nan n_roi, then per ROI: label n and n lines x y intensity, then n_roi lines of 46 values" in enum order
// (IH_MEAN_VAL .. IH_BIN_SIZE).
#include <cmath>
#include <cstdio>
#include <cstring>
#include "nyxhip_feature_method.hpp"

using namespace NyxusHip;

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--compile-check")) {
        static_assert((int)Feature2D::IH_BIN_SIZE - (int)Feature2D::IH_MEAN_VAL == NYXHIP_IH_COLS - 1 &&
                      (int)Feature2D::IH_ROBUST_MEAN_VAL - (int)Feature2D::IH_MEAN_VAL == 19 && (int)Feature2D::IH_MEAN_IDX - (int)Feature2D::IH_MEAN_VAL == 20 &&
                      (int)Feature2D::IH_MAX_GRADIENT - (int)Feature2D::IH_MEAN_VAL == 39 && (int)Feature2D::IH_BIN_SIZE + 1 == (int)Feature2D::_COUNT_,
                      "46 contiguous codes in enum order, at the end of the enum");
        printf("compiled\n");
        return 0;
    }
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int depth = 0, n_roi = 0;
    double soft_nan = 0.0;
    if (fscanf(f, "%d %lf %d", &depth, &soft_nan, &n_roi) != 3) return 2;
    std::unordered_map<int, LR> roiData;
    std::vector<int> L;
    for (int k = 0; k < n_roi; k++) {
        int label = 0, n = 0;
        if (fscanf(f, "%d %d", &label, &n) != 2) return 2;
        LR& r = roiData[label];
        r.label = label;
        for (int i = 0; i < n; i++) {
            long x, y; unsigned v;
            if (fscanf(f, "%ld %ld %u", &x, &y, &v) != 3) return 2;
            r.feed_pixel(x, y, v);
        }
        r.initialize_fvals();
        L.push_back(label);
    }
    std::vector<double> want((size_t)n_roi * 46);
    for (double& v : want) if (fscanf(f, "%lf", &v) != 1) return 2;
    fclose(f);
    Fsettings s((size_t)NyxSetting::__COUNT__);
    s[(int)NyxSetting::SOFTNAN].rval = soft_nan;
    s[(int)NyxSetting::TINY].rval = 1e-10;
    s[(int)NyxSetting::GREYDEPTH].ival = depth;
    s[(int)NyxSetting::GLCM_GREYDEPTH].ival = depth;
    s[(int)NyxSetting::GLCM_OFFSET].ival = 1;
    s[(int)NyxSetting::IBSI].bval = true;
    Dataset ds;
    runParallel(IntensityHistogramFeatures::reduce, 4, 1, L.size(), &L, &roiData, s, ds);
    const int e0 = (int)Feature2D::IH_ENTROPY_VAL - (int)Feature2D::IH_MEAN_VAL, e1 = (int)Feature2D::IH_ENTROPY_IDX - (int)Feature2D::IH_MEAN_VAL;
    int bad = 0;
    auto cmp = [&](int roi, int c, double got, double w) {
        const bool both_nan = std::isnan(got) && std::isnan(w);
        const bool ok = both_nan || ((c == e0 || c == e1) ? std::fabs(got - w) <= 1e-5 * std::fabs(w) : got == w);
        if (!ok) { printf("ROI %d code %d: got %.17g want %.17g\n", roi, c, got, w); bad++; }
    };
    for (int k = 0; k < n_roi; k++)
        for (int c = 0; c < 46; c++) {
            const std::vector<double>& fv = roiData[L[k]].fvals[(int)Feature2D::IH_MEAN_VAL + c];
            if (fv.size() != 1) { printf("ROI %d code %d: %zu values\n", L[k], c, fv.size()); return 1; }
            cmp(L[k], c, fv[0], want[(size_t)k * 46 + c]);
        }
    // one ROI through calculate() / save_value()
    IntensityHistogramFeatures one;
    std::vector<std::vector<double>> fv;
    one.calculate(roiData[L[0]], s);
    one.save_value(fv);
    for (int c = 0; c < 46; c++) cmp(-1, c, fv[(int)Feature2D::IH_MEAN_VAL + c][0], want[c]);
    // IBSI off: the class gates itself
    s[(int)NyxSetting::IBSI].bval = false;
    IntensityHistogramFeatures::extract(roiData[L[0]], s);
    for (int c = 0; c < 46; c++)
        if (roiData[L[0]].fvals[(int)Feature2D::IH_MEAN_VAL + c][0] != soft_nan) { printf("gate: code %d\n", c); bad++; }
    FeatureSet fs;
    fs.enableFeature(Feature2D::IH_P90_IDX);
    if (!IntensityHistogramFeatures::required(fs) || PixelIntensityFeatures::required(fs) || Imoms2D_feature::required(fs) || NeighborsFeature::required(fs)) { printf("required()\n"); bad++; }
    FeatureSet fs2;
    fs2.enableFeature(Feature2D::IMOM_WHU7);
    fs2.enableFeature(Feature2D::ANG_BW_NEIGHBORS_MODE);
    if (IntensityHistogramFeatures::required(fs2) || !one.provides((int)Feature2D::IH_BIN_SIZE) || one.provides((int)Feature2D::IMOM_WHU7)) { printf("required() 2\n"); bad++; }
    if (!bad) printf("ALL PASSED\n");
    return bad ? 1 : 0;
}
