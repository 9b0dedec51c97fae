// test_outline_method.cpp -- FractalDimensionFeature, EulerNumberFeature and RoiRadiusFeature of include/nyxhip_feature_method.hpp,
// used the way the reference's unit tests use its classes: build an LR from a pixel list, calculate(), save_value(), compare with
// the recorded values.  Input: a text file "n, then n lines x y intensity, then 6 values" (FRACT_DIM_BOXCOUNT, FRACT_DIM_PERIMETER,
// EULER_NUMBER, ROI_RADIUS_MEAN, ROI_RADIUS_MAX, ROI_RADIUS_MEDIAN).
#include <cmath>
#include <cstdio>
#include <cstring>
#include "nyxhip_feature_method.hpp"

using namespace NyxusHip;

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--compile-check")) {
        static_assert((int)Feature2D::FRACT_DIM_BOXCOUNT == (int)Feature2D::UNIFORMITY_PIU + 1 && (int)Feature2D::GLCM_ASM == (int)Feature2D::ROI_RADIUS_MEDIAN + 1,
                      "the six codes sit between the intensity block and GLCM");
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
    double want[6];
    for (int i = 0; i < 6; i++) if (fscanf(f, "%lf", &want[i]) != 1) return 2;
    fclose(f);
    r.initialize_fvals();
    Fsettings s;
    FractalDimensionFeature fd;
    fd.calculate(r, s);
    fd.save_value(r.fvals);
    EulerNumberFeature::extract(r, s);
    RoiRadiusFeature rr;
    rr.calculate(r, s);
    rr.save_value(r.fvals);
    const Feature2D codes[6] = {Feature2D::FRACT_DIM_BOXCOUNT, Feature2D::FRACT_DIM_PERIMETER, Feature2D::EULER_NUMBER,
                                Feature2D::ROI_RADIUS_MEAN, Feature2D::ROI_RADIUS_MAX, Feature2D::ROI_RADIUS_MEDIAN};
    int bad = 0;
    for (int c = 0; c < 6; c++) {
        if (r.fvals[(int)codes[c]].size() != 1) { printf("code %d: %zu values\n", c, r.fvals[(int)codes[c]].size()); return 1; }
        const double got = r.fvals[(int)codes[c]][0];
        const bool exact = c == 2 || c == 4 || c == 5;
        const bool ok = exact ? got == want[c] : std::fabs(got - want[c]) <= 1e-5 * std::fabs(want[c]) || (c < 2 && std::fabs(got - want[c]) <= 1e-5);
        if (!ok) { printf("code %d: got %.17g want %.17g\n", c, got, want[c]); bad++; }
    }
    // the fused ladder picks the families up from the feature set
    FeatureSet fs;
    fs.enableFeature(Feature2D::ROI_RADIUS_MAX);
    fs.enableFeature(Feature2D::EULER_NUMBER);
    if (!RoiRadiusFeature::required(fs) || !EulerNumberFeature::required(fs) || FractalDimensionFeature::required(fs) || GLCMFeature::required(fs) ||
        PixelIntensityFeatures::required(fs)) { printf("required() ladder\n"); bad++; }
    if (!bad) printf("ALL PASSED\n");
    return bad ? 1 : 0;
}
