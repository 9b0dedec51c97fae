// test_circle_method.cpp -- EnclosingInscribingCircumscribingCircleFeature and GeodeticLengthThicknessFeature of
// include/nyxhip_feature_method.hpp, used the way the reference's unit tests use its classes: build an LR from a pixel list at its
// ABSOLUTE position (the adapter hands LR::aabb's origin to nyxhip_featurize_batch_at), calculate(), save_value(), compare with the
// recorded values.  Input: a text file "n, then n lines x y intensity, then 5 values" in enum order (DIAMETER_MIN_ENCLOSING_CIRCLE,
// DIAMETER_CIRCUMSCRIBING_CIRCLE, DIAMETER_INSCRIBING_CIRCLE, GEODETIC_LENGTH, THICKNESS).
#include <cmath>
#include <cstdio>
#include <cstring>
#include "nyxhip_feature_method.hpp"

using namespace NyxusHip;

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--compile-check")) {
        static_assert((int)Feature2D::DIAMETER_INSCRIBING_CIRCLE - (int)Feature2D::DIAMETER_MIN_ENCLOSING_CIRCLE == 2 &&
                      (int)Feature2D::GEODETIC_LENGTH - (int)Feature2D::DIAMETER_MIN_ENCLOSING_CIRCLE == 3 &&
                      (int)Feature2D::THICKNESS - (int)Feature2D::GEODETIC_LENGTH == 1, "five contiguous codes, the circles first");
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
    double want[5];
    for (int i = 0; i < 5; i++) if (fscanf(f, "%lf", &want[i]) != 1) return 2;
    fclose(f);
    r.initialize_fvals();
    Fsettings s;
    EnclosingInscribingCircumscribingCircleFeature ci;
    ci.calculate(r, s);
    ci.save_value(r.fvals);
    GeodeticLengthThicknessFeature ge;
    ge.calculate(r, s);
    ge.save_value(r.fvals);
    int bad = 0;
    for (int c = 0; c < 5; c++) {
        const int code = (int)Feature2D::DIAMETER_MIN_ENCLOSING_CIRCLE + c;
        if (r.fvals[code].size() != 1) { printf("code %d: %zu values\n", c, r.fvals[code].size()); return 1; }
        const double got = r.fvals[code][0];
        if (!(std::fabs(got - want[c]) <= 1e-5 * std::fabs(want[c])) || !std::isfinite(got)) { printf("code %d: got %.17g want %.17g\n", c, got, want[c]); bad++; }
    }
    // extract() gives the same values
    LR r2 = r;
    r2.initialize_fvals();
    EnclosingInscribingCircumscribingCircleFeature::extract(r2, s);
    GeodeticLengthThicknessFeature::extract(r2, s);
    for (int c = 0; c < 5; c++)
        if (r2.fvals[(int)Feature2D::DIAMETER_MIN_ENCLOSING_CIRCLE + c][0] != r.fvals[(int)Feature2D::DIAMETER_MIN_ENCLOSING_CIRCLE + c][0]) { printf("extract(): code %d\n", c); bad++; }
    // the fused ladder picks the families up from the feature set
    FeatureSet fs;
    fs.enableFeature(Feature2D::DIAMETER_INSCRIBING_CIRCLE);
    if (!EnclosingInscribingCircumscribingCircleFeature::required(fs) || GeodeticLengthThicknessFeature::required(fs) || EulerNumberFeature::required(fs) ||
        RoiRadiusFeature::required(fs)) { printf("required() ladder\n"); bad++; }
    FeatureSet fs2;
    fs2.enableFeature(Feature2D::THICKNESS);
    if (EnclosingInscribingCircumscribingCircleFeature::required(fs2) || !GeodeticLengthThicknessFeature::required(fs2)) { printf("required() ladder 2\n"); bad++; }
    if (!bad) printf("ALL PASSED\n");
    return bad ? 1 : 0;
}
