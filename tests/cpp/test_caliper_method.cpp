// test_caliper_method.cpp -- CaliperFeretFeature, CaliperMartinFeature and CaliperNassensteinFeature of
// include/nyxhip_feature_method.hpp, used the way the reference's unit tests use its classes: build an LR from a pixel list at its
// ABSOLUTE position (the adapter hands LR::aabb's origin to nyxhip_featurize_batch_at), calculate(), save_value(), compare with the
// recorded values.  Input: a text file "n, then n lines x y intensity, then 20 values" in enum order (MIN_FERET_ANGLE ..
// STAT_NASSENSTEIN_DIAM_MODE).
#include <cmath>
#include <cstdio>
#include <cstring>
#include "nyxhip_feature_method.hpp"

using namespace NyxusHip;

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--compile-check")) {
        static_assert((int)Feature2D::MIN_FERET_ANGLE == (int)Feature2D::FRACT_DIM_PERIMETER + 1 &&
                      (int)Feature2D::EULER_NUMBER == (int)Feature2D::STAT_NASSENSTEIN_DIAM_MODE + 1 &&
                      (int)Feature2D::STAT_NASSENSTEIN_DIAM_MODE - (int)Feature2D::MIN_FERET_ANGLE == 19,
                      "the twenty codes sit between FRACT_DIM_PERIMETER and EULER_NUMBER");
        printf("compiled\n");
        return 0;
    }
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n = 0;
    if (fscanf(f, "%d", &n) != 1) return 2;
    LR r(101);
    for (int i = 0; i < n; i++) {
        long x, y; unsigned v;
        if (fscanf(f, "%ld %ld %u", &x, &y, &v) != 3) return 2;
        r.feed_pixel(x, y, v);
    }
    double want[20];
    for (int i = 0; i < 20; i++) if (fscanf(f, "%lf", &want[i]) != 1) return 2;
    fclose(f);
    if (r.aabb.get_xmin() == 0 && r.aabb.get_ymin() == 0) { printf("the case must lie away from the origin\n"); return 2; }
    r.initialize_fvals();
    Fsettings s;
    CaliperFeretFeature fe;
    fe.calculate(r, s);
    fe.save_value(r.fvals);
    CaliperMartinFeature::extract(r, s);
    CaliperNassensteinFeature na;
    na.calculate(r, s);
    na.save_value(r.fvals);
    int bad = 0;
    for (int c = 0; c < 20; c++) {
        const int code = (int)Feature2D::MIN_FERET_ANGLE + c;
        if (r.fvals[code].size() != 1) { printf("code %d: %zu values\n", c, r.fvals[code].size()); return 1; }
        const double got = r.fvals[code][0];
        const bool exact = c == 0 || c == 1 || c == 7 || c == 13 || c == 19;      // the angles and the modes
        const bool ok = exact ? got == want[c] : std::fabs(got - want[c]) <= 1e-5 * std::fabs(want[c]);
        if (!ok) { printf("code %d: got %.17g want %.17g\n", c, got, want[c]); bad++; }
    }
    // the fused ladder picks the families up from the feature set
    FeatureSet fs;
    fs.enableFeature(Feature2D::STAT_MARTIN_DIAM_MEDIAN);
    fs.enableFeature(Feature2D::MAX_FERET_ANGLE);
    if (!CaliperMartinFeature::required(fs) || !CaliperFeretFeature::required(fs) || CaliperNassensteinFeature::required(fs) ||
        EulerNumberFeature::required(fs) || FractalDimensionFeature::required(fs)) { printf("required() ladder\n"); bad++; }
    if (!bad) printf("ALL PASSED\n");
    return bad ? 1 : 0;
}
