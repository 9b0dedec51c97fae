// test_hexpoly_method.cpp -- HexagonalityPolygonalityFeature of include/nyxhip_feature_method.hpp, used the way the reference's workflow
// uses its class: the ROIs of one image as LRs at their ABSOLUTE positions in a Roidata,
// HexagonalityPolygonalityFeature::manual_reduce(roiData, settings, uniqueLabels) with PIXELDISTANCE in the settings, then the three fvals
// of every ROI against the recorded values, bit for bit.
// Input: a text file "radius n_roi, then per ROI: label n and n lines x y intensity, then n_roi lines of 3 values" in the order of the
// ROIs and enum order (POLYGONALITY_AVE, HEXAGONALITY_AVE, HEXAGONALITY_STDDEV).
#include <cmath>
#include <cstdio>
#include <cstring>
#include "nyxhip_feature_method.hpp"

using namespace NyxusHip;

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--compile-check")) {
        static_assert((int)FeatureHexPoly::POLYGONALITY_AVE == (int)FeatureIMQ::_COUNT_ && (int)FeatureHexPoly::_FIRST_ == (int)FeatureHexPoly::POLYGONALITY_AVE &&
                      (int)FeatureHexPoly::HEXAGONALITY_AVE - (int)FeatureHexPoly::POLYGONALITY_AVE == 1 &&
                      (int)FeatureHexPoly::HEXAGONALITY_STDDEV - (int)FeatureHexPoly::POLYGONALITY_AVE == 2 &&
                      (int)FeatureHexPoly::_COUNT_ - (int)FeatureHexPoly::_FIRST_ == NYXHIP_HEXPOLY_COLS &&
                      HexagonalityPolygonalityFeature::novalue == -1, "three contiguous codes in enum order behind the image-quality codes");
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
    std::vector<double> want((size_t)n_roi * 3);
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
    HexagonalityPolygonalityFeature::manual_reduce(roiData, s, uniq);
    int bad = 0, gated = 0;
    for (int k = 0; k < n_roi; k++)
        for (int c = 0; c < 3; c++) {
            const std::vector<double>& fv = roiData[order[k]].fvals[(int)FeatureHexPoly::_FIRST_ + c];
            if (fv.size() != 1) { printf("ROI %d code %d: %zu values\n", order[k], c, fv.size()); return 1; }
            const double got = fv[0], w = want[(size_t)k * 3 + c];
            if (got == -1.0) gated++;
            if (!(got == w)) { printf("ROI %d code %d: got %.17g want %.17g\n", order[k], c, got, w); bad++; }
        }
    if (gated == 0 || gated == 3 * n_roi) { printf("the case must hold gated and served rows (%d of %d values are -1)\n", gated, 3 * n_roi); bad++; }
    FeatureSet fs;
    fs.enableFeature(FeatureHexPoly::HEXAGONALITY_AVE);
    if (!HexagonalityPolygonalityFeature::required(fs) || NeighborsFeature::required(fs) || CaliperFeretFeature::required(fs)) { printf("required()\n"); bad++; }
    FeatureSet fs2;
    fs2.enableFeature(Feature2D::NUM_NEIGHBORS);
    if (HexagonalityPolygonalityFeature::required(fs2)) { printf("required() 2\n"); bad++; }
    HexagonalityPolygonalityFeature hp;
    if (!hp.provides((int)FeatureHexPoly::HEXAGONALITY_STDDEV) || hp.provides((int)Feature2D::NUM_NEIGHBORS)) { printf("provides()\n"); bad++; }
    if (!bad) printf("ALL PASSED\n");
    return bad ? 1 : 0;
}
