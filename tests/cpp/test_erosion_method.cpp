// test_erosion_method.cpp -- EllipseFittingFeature and ErosionPixelsFeature of include/nyxhip_feature_method.hpp, used the way the
// reference's unit tests use its classes: build an LR from a pixel list, calculate(), save_value(), compare with the recorded values.
// Input: a text file "n, then n lines x y intensity, then 8 values, then 8 flags (1: compared)" in enum order
// (MAJOR_AXIS_LENGTH .. ROUNDNESS, EROSIONS_2_VANISH, EROSIONS_2_VANISH_COMPLEMENT).
#include <cmath>
#include <cstdio>
#include <cstring>
#include "nyxhip_feature_method.hpp"

using namespace NyxusHip;

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--compile-check")) {
        static_assert((int)Feature2D::ROUNDNESS - (int)Feature2D::MAJOR_AXIS_LENGTH == 5 &&
                      (int)Feature2D::EROSIONS_2_VANISH - (int)Feature2D::MAJOR_AXIS_LENGTH == 6 &&
                      (int)Feature2D::EROSIONS_2_VANISH_COMPLEMENT - (int)Feature2D::EROSIONS_2_VANISH == 1, "eight contiguous codes, the ellipse first");
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
    double want[8];
    int cmp[8];
    for (int i = 0; i < 8; i++) if (fscanf(f, "%lf", &want[i]) != 1) return 2;
    for (int i = 0; i < 8; i++) if (fscanf(f, "%d", &cmp[i]) != 1) return 2;
    fclose(f);
    r.initialize_fvals();
    Fsettings s;
    EllipseFittingFeature el;
    el.calculate(r, s);
    el.save_value(r.fvals);
    ErosionPixelsFeature er;
    er.calculate(r, s);
    er.save_value(r.fvals);
    int bad = 0;
    for (int c = 0; c < 8; c++) {
        const int code = (int)Feature2D::MAJOR_AXIS_LENGTH + c;
        if (r.fvals[code].size() != 1) { printf("code %d: %zu values\n", c, r.fvals[code].size()); return 1; }
        const double got = r.fvals[code][0];
        const bool ok = c >= 6 ? got == want[c] : (!cmp[c] || std::fabs(got - want[c]) <= 1e-5 * std::fabs(want[c]));
        if (!ok || !std::isfinite(got)) { printf("code %d: got %.17g want %.17g\n", c, got, want[c]); bad++; }
    }
    // extract() gives the same values
    LR r2 = r;
    r2.initialize_fvals();
    EllipseFittingFeature::extract(r2, s);
    ErosionPixelsFeature::extract(r2, s);
    for (int c = 0; c < 8; c++)
        if (r2.fvals[(int)Feature2D::MAJOR_AXIS_LENGTH + c][0] != r.fvals[(int)Feature2D::MAJOR_AXIS_LENGTH + c][0]) { printf("extract(): code %d\n", c); bad++; }
    // the fused ladder picks the families up from the feature set
    FeatureSet fs;
    fs.enableFeature(Feature2D::ORIENTATION);
    if (!EllipseFittingFeature::required(fs) || ErosionPixelsFeature::required(fs) || ChordsFeature::required(fs) || FractalDimensionFeature::required(fs)) { printf("required() ladder\n"); bad++; }
    FeatureSet fs2;
    fs2.enableFeature(Feature2D::EROSIONS_2_VANISH);
    if (EllipseFittingFeature::required(fs2) || !ErosionPixelsFeature::required(fs2)) { printf("required() ladder 2\n"); bad++; }
    if (!bad) printf("ALL PASSED\n");
    return bad ? 1 : 0;
}
