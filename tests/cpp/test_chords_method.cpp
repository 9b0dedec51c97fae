// test_chords_method.cpp -- ChordsFeature of include/nyxhip_feature_method.hpp, used the way the reference's unit tests use its
// classes: build an LR from a pixel list at its ABSOLUTE position (the adapter hands LR::aabb's origin to nyxhip_featurize_batch_at),
// calculate(), save_value(), compare with the recorded values.  Input: a text file "n, then n lines x y intensity, then 16 values"
// in enum order (MAXCHORDS_MAX .. ALLCHORDS_STDDEV).
#include <cmath>
#include <cstdio>
#include <cstring>
#include "nyxhip_feature_method.hpp"

using namespace NyxusHip;

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--compile-check")) {
        static_assert((int)Feature2D::ALLCHORDS_STDDEV - (int)Feature2D::MAXCHORDS_MAX == 15 &&
                      (int)Feature2D::ALLCHORDS_MAX - (int)Feature2D::MAXCHORDS_MAX == 8, "sixteen contiguous codes, MAXCHORDS first");
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
    double want[16];
    for (int i = 0; i < 16; i++) if (fscanf(f, "%lf", &want[i]) != 1) return 2;
    fclose(f);
    if (r.aabb.get_xmin() == 0 && r.aabb.get_ymin() == 0) { printf("the case must lie away from the origin\n"); return 2; }
    r.initialize_fvals();
    Fsettings s;
    ChordsFeature ch;
    ch.calculate(r, s);
    ch.save_value(r.fvals);
    int bad = 0;
    for (int c = 0; c < 16; c++) {
        const int code = (int)Feature2D::MAXCHORDS_MAX + c;
        if (r.fvals[code].size() != 1) { printf("code %d: %zu values\n", c, r.fvals[code].size()); return 1; }
        const double got = r.fvals[code][0];
        const bool approx = (c & 7) == 5 || (c & 7) == 7;                         // MEAN and STDDEV; everything else exactly
        const bool ok = approx ? std::fabs(got - want[c]) <= 1e-5 * std::fabs(want[c]) : got == want[c];
        if (!ok) { printf("code %d: got %.17g want %.17g\n", c, got, want[c]); bad++; }
    }
    // extract() gives the same values
    LR r2 = r;
    r2.initialize_fvals();
    ChordsFeature::extract(r2, s);
    for (int c = 0; c < 16; c++)
        if (r2.fvals[(int)Feature2D::MAXCHORDS_MAX + c][0] != r.fvals[(int)Feature2D::MAXCHORDS_MAX + c][0]) { printf("extract(): code %d\n", c); bad++; }
    // the fused ladder picks the family up from the feature set
    FeatureSet fs;
    fs.enableFeature(Feature2D::ALLCHORDS_MEDIAN);
    if (!ChordsFeature::required(fs) || CaliperNassensteinFeature::required(fs) || EulerNumberFeature::required(fs)) { printf("required() ladder\n"); bad++; }
    if (!bad) printf("ALL PASSED\n");
    return bad ? 1 : 0;
}
