// test_imq_method.cpp -- FocusScoreFeature and SaturationFeature of include/nyxhip_feature_method.hpp, used the way the reference's workflow
// uses its classes: LRs fed pixel by pixel, runParallel(F::parallel_process_1_batch, ...), then the four FeatureIMQ values of every ROI against
// the recorded values; calculate() + save_value() on one ROI; required(); reduce_trivial_rois_manual().
// Input: a text file "soft_nan n_roi, then per ROI: label n and n lines x y intensity, then n_roi lines of 4 values" in enum order
// (FOCUS_SCORE, LOCAL_FOCUS_SCORE, MAX_SATURATION, MIN_SATURATION).
#include <cmath>
#include <cstdio>
#include <cstring>
#include "nyxhip_feature_method.hpp"

using namespace NyxusHip;

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--compile-check")) {
        static_assert((int)FeatureIMQ::FOCUS_SCORE == (int)Feature2D::_COUNT_ && (int)FeatureIMQ::_FIRST_ == (int)FeatureIMQ::FOCUS_SCORE &&
                      (int)FeatureIMQ::LOCAL_FOCUS_SCORE - (int)FeatureIMQ::FOCUS_SCORE == 1 && (int)FeatureIMQ::POWER_SPECTRUM_SLOPE - (int)FeatureIMQ::FOCUS_SCORE == 2 &&
                      (int)FeatureIMQ::MAX_SATURATION - (int)FeatureIMQ::FOCUS_SCORE == 3 && (int)FeatureIMQ::MIN_SATURATION - (int)FeatureIMQ::FOCUS_SCORE == 4 &&
                      (int)FeatureIMQ::SHARPNESS - (int)FeatureIMQ::FOCUS_SCORE == 5 && (int)FeatureIMQ::_COUNT_ - (int)FeatureIMQ::FOCUS_SCORE == 6 &&
                      (int)Feature2D::IH_BIN_SIZE + 1 == (int)Feature2D::_COUNT_ && NYXHIP_IMQ_COLS == 4,
                      "the six codes of the reference's enum, in its order, behind every Feature2D code");
        printf("compiled\n");
        return 0;
    }
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n_roi = 0;
    double soft_nan = 0.0;
    if (fscanf(f, "%lf %d", &soft_nan, &n_roi) != 2) return 2;
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
            r.feed_pixel(x + 100, y + 7, v);                 // anywhere in the image: the classes read the box, not its place
        }
        r.initialize_fvals();
        L.push_back(label);
    }
    std::vector<double> want((size_t)n_roi * 4);
    for (double& v : want) if (fscanf(f, "%lf", &v) != 1) return 2;
    fclose(f);
    Fsettings s((size_t)NyxSetting::__COUNT__);
    s[(int)NyxSetting::SOFTNAN].rval = soft_nan;
    s[(int)NyxSetting::TINY].rval = 1e-10;
    s[(int)NyxSetting::GREYDEPTH].ival = 256;
    s[(int)NyxSetting::GLCM_GREYDEPTH].ival = 256;
    s[(int)NyxSetting::GLCM_OFFSET].ival = 1;
    Dataset ds;
    static const FeatureIMQ codes[4] = {FeatureIMQ::FOCUS_SCORE, FeatureIMQ::LOCAL_FOCUS_SCORE, FeatureIMQ::MAX_SATURATION, FeatureIMQ::MIN_SATURATION};
    int bad = 0;
    auto cmp = [&](int roi, int c, double got, double w) {
        const bool ok = c >= 2 ? got == w : (w == 0.0 ? got == 0.0 : std::fabs(got - w) <= 1e-5 * std::fabs(w));   // saturation: bit for bit
        if (!ok) { printf("ROI %d code %d: got %.17g want %.17g\n", roi, c, got, w); bad++; }
    };
    auto check_all = [&](const char* tag) {
        for (int k = 0; k < n_roi; k++)
            for (int c = 0; c < 4; c++) {
                const std::vector<double>& fv = roiData[L[k]].fvals[(int)codes[c]];
                if (fv.size() != 1) { printf("%s: ROI %d code %d: %zu values\n", tag, L[k], c, fv.size()); bad++; continue; }
                cmp(L[k], c, fv[0], want[(size_t)k * 4 + c]);
            }
    };
    runParallel(FocusScoreFeature::parallel_process_1_batch, 4, 1, L.size(), &L, &roiData, s, ds);
    runParallel(SaturationFeature::parallel_process_1_batch, 4, 1, L.size(), &L, &roiData, s, ds);
    check_all("runParallel");
    if (roiData[L[0]].fvals[(int)FeatureIMQ::POWER_SPECTRUM_SLOPE][0] != 0.0 || roiData[L[0]].fvals[(int)FeatureIMQ::SHARPNESS][0] != 0.0) { printf("unserved codes written\n"); bad++; }
    // one ROI through calculate() / save_value(): each class saves its own two codes
    FocusScoreFeature fo;
    SaturationFeature sa;
    std::vector<std::vector<double>> fv;
    fo.calculate(roiData[L[0]], s);
    fo.save_value(fv);
    if (fv.size() != (size_t)FeatureIMQ::_COUNT_ || fv[(int)FeatureIMQ::MAX_SATURATION][0] != 0.0) { printf("save_value of FocusScoreFeature\n"); bad++; }
    sa.calculate(roiData[L[0]], s);
    sa.save_value(fv);
    for (int c = 0; c < 4; c++) cmp(-1, c, fv[(int)codes[c]][0], want[c]);
    // required(): each class by its own codes only
    FeatureSet fs;
    fs.enableFeature(FeatureIMQ::LOCAL_FOCUS_SCORE);
    if (!FocusScoreFeature::required(fs) || SaturationFeature::required(fs) || PixelIntensityFeatures::required(fs) || IntensityHistogramFeatures::required(fs)) { printf("required()\n"); bad++; }
    FeatureSet fs2;
    fs2.enableFeatures({FeatureIMQ::MIN_SATURATION, FeatureIMQ::SHARPNESS});
    fs2.enableFeature(Feature2D::IH_BIN_SIZE);
    if (FocusScoreFeature::required(fs2) || !SaturationFeature::required(fs2) || !fo.provides((int)FeatureIMQ::FOCUS_SCORE) || fo.provides((int)FeatureIMQ::MAX_SATURATION) ||
        !sa.provides((int)FeatureIMQ::MIN_SATURATION) || sa.provides((int)FeatureIMQ::SHARPNESS)) { printf("required() 2\n"); bad++; }
    // the manual reduce: the two classes beside a family
    for (int l : L) roiData[l].initialize_fvals();
    FeatureSet all;
    all.enableFeatures({FeatureIMQ::FOCUS_SCORE, FeatureIMQ::MAX_SATURATION});
    all.enableFeature(Feature2D::MEAN);
    reduce_trivial_rois_manual(L, roiData, all, s, ds);
    check_all("reduce_trivial_rois_manual");
    if (!(roiData[L[0]].fvals[(int)Feature2D::MEAN][0] > 0.0)) { printf("MEAN beside the image-quality classes\n"); bad++; }
    if (!bad) printf("ALL PASSED\n");
    return bad ? 1 : 0;
}
