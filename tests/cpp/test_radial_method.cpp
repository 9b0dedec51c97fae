// test_radial_method.cpp -- RadialDistributionFeature of include/nyxhip_feature_method.hpp, used the way the reference's unit test
// uses its class (tests/test_2d_radial_regression.h:55-75): build an LR from a pixel list, calculate(), save_value(), compare
// FRAC_AT_D / MEAN_FRAC / RADIAL_CV with the recorded vector.  Input: a text file "n, then n lines x y intensity, then 24 values".
#include <cmath>
#include <cstdio>
#include <cstring>
#include "nyxhip_feature_method.hpp"

using namespace NyxusHip;

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--compile-check")) { printf("compiled\n"); return 0; }
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
    double want[24];
    for (int i = 0; i < 24; i++) if (fscanf(f, "%lf", &want[i]) != 1) return 2;
    fclose(f);
    r.initialize_fvals();
    Fsettings s;
    RadialDistributionFeature radial;
    radial.calculate(r, s);
    radial.save_value(r.fvals);
    const Feature2D codes[3] = {Feature2D::FRAC_AT_D, Feature2D::MEAN_FRAC, Feature2D::RADIAL_CV};
    int bad = 0;
    for (int c = 0; c < 3; c++) {
        if (r.fvals[(int)codes[c]].size() != 8) { printf("code %d: %zu values\n", c, r.fvals[(int)codes[c]].size()); return 1; }
        for (int i = 0; i < 8; i++)
            if (!(std::fabs(r.fvals[(int)codes[c]][i] - want[c * 8 + i]) <= 1e-9)) { printf("code %d bin %d: got %.17g want %.17g\n", c, i, r.fvals[(int)codes[c]][i], want[c * 8 + i]); bad++; }
    }
    // the fused ladder picks the family up from the feature set
    FeatureSet fs;
    fs.enableFeature(Feature2D::RADIAL_CV);
    if (!RadialDistributionFeature::required(fs) || GaborFeature::required(fs)) { printf("required() ladder\n"); bad++; }
    if (!bad) printf("ALL PASSED\n");
    return bad ? 1 : 0;
}
