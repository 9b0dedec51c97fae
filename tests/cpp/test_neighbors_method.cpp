// test_neighbors_method.cpp -- NeighborsFeature of include/nyxhip_feature_method.hpp, used the way the reference's workflow uses its
// class: the ROIs of one image as LRs at their ABSOLUTE positions in a Roidata, NeighborsFeature::manual_reduce(roiData, settings,
// uniqueLabels) with PIXELDISTANCE in the settings, then the nine fvals of every ROI against the recorded values.
// Input: a text file "radius n_roi, then per ROI: label n and n lines x y intensity, then n_roi lines of 9 values" in ascending label
// order and enum order (NUM_NEIGHBORS .. ANG_BW_NEIGHBORS_MODE).
#include <cmath>
#include <cstdio>
#include <cstring>
#include "nyxhip_feature_method.hpp"

using namespace NyxusHip;

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--compile-check")) {
        static_assert((int)Feature2D::ANG_BW_NEIGHBORS_MODE - (int)Feature2D::NUM_NEIGHBORS == NYXHIP_NEIGHBOR_COLS - 1 &&
                      (int)Feature2D::PERCENT_TOUCHING - (int)Feature2D::NUM_NEIGHBORS == 1 &&
                      (int)Feature2D::CLOSEST_NEIGHBOR2_ANG - (int)Feature2D::CLOSEST_NEIGHBOR1_DIST == 3, "nine contiguous codes in enum order");
        printf("compiled\n");
        return 0;
    }
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int radius = 0, n_roi = 0;
    if (fscanf(f, "%d %d", &radius, &n_roi) != 2) return 2;
    Roidata roiData;
    std::unordered_set<int> uniq;
    std::vector<int> order;
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
        uniq.insert(label);
        order.push_back(label);
    }
    std::vector<double> want((size_t)n_roi * 9);
    for (double& v : want) if (fscanf(f, "%lf", &v) != 1) return 2;
    fclose(f);
    Fsettings s((size_t)NyxSetting::__COUNT__);
    s[(int)NyxSetting::SOFTNAN].rval = 0.0;
    s[(int)NyxSetting::TINY].rval = 1e-10;
    s[(int)NyxSetting::GREYDEPTH].ival = 64;
    s[(int)NyxSetting::GLCM_GREYDEPTH].ival = 64;
    s[(int)NyxSetting::GLCM_OFFSET].ival = 1;
    s[(int)NyxSetting::IBSI].bval = false;
    s[(int)NyxSetting::PIXELDISTANCE].ival = radius;
    NeighborsFeature::manual_reduce(roiData, s, uniq);
    static const bool exact[9] = {true, true, true, false, true, false, false, false, true};
    int bad = 0;
    for (int k = 0; k < n_roi; k++)
        for (int c = 0; c < 9; c++) {
            const std::vector<double>& fv = roiData[order[k]].fvals[(int)Feature2D::NUM_NEIGHBORS + c];
            if (fv.size() != 1) { printf("ROI %d code %d: %zu values\n", order[k], c, fv.size()); return 1; }
            const double got = fv[0], w = want[(size_t)k * 9 + c];
            const bool ok = exact[c] ? got == w : std::fabs(got - w) <= 1e-5 * std::fabs(w);
            if (!ok || !std::isfinite(got)) { printf("ROI %d code %d: got %.17g want %.17g\n", order[k], c, got, w); bad++; }
        }
    FeatureSet fs;
    fs.enableFeature(Feature2D::PERCENT_TOUCHING);
    if (!NeighborsFeature::required(fs) || RoiRadiusFeature::required(fs) || GLCMFeature::required(fs)) { printf("required()\n"); bad++; }
    FeatureSet fs2;
    fs2.enableFeature(Feature2D::ROI_RADIUS_MEDIAN);
    if (NeighborsFeature::required(fs2)) { printf("required() 2\n"); bad++; }
    if (!bad) printf("ALL PASSED\n");
    return bad ? 1 : 0;
}
