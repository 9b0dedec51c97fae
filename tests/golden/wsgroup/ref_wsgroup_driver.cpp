/*
 * ref_wsgroup_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp and tests/golden/radial/ref_radial_driver.cpp) around the
 * reference's own ContourFeature, Smoms2D_feature, Imoms2D_feature and RadialDistributionFeature classes in WHOLE-SLIDE mode
 * (fst[SINGLEROI] = true).  make_wsgroup_golden.py compiles it OUTSIDE the repository against the reference sources where they lie
 * and records what it returns into the fixtures next to this file; nothing compiled from it is kept.
 *
 * One slide of w x h pixels (uint32, row-major): the LR the reference's whole-slide workflow builds (workflow_2d_whole.cpp:36-213) --
 * raw_pixels in row-major order, zeros included; aabb (0,0)-(w-1,h-1); aux_min / aux_max over all pixels -- then the ladder
 * ContourFeature::reduce, Smoms2D, Imoms2D, RadialDistributionFeature (reduce_trivial_rois.cpp).
 *   out[0 .. 7)      PERIMETER .. EDGE_INTEGRATED_INTENSITY
 *   out[7 .. 97)     SPAT_MOMENT_00 .. WEIGHTED_HU_M7
 *   out[97 .. 187)   IMOM_RM_00 .. IMOM_WHU7
 *   out[187 .. 211)  FRAC_AT_D[8] | MEAN_FRAC[8] | RADIAL_CV[8]
 *   info[0]          pixels (not aligned with a corner) whose min of the four dist_to_segment differs from min(x, w-1-x, y, h-1-y)
 *   info[1]          max_sqdist of the centre pixel over the four corners (0: the reference's undefined case, a 1 x 1 slide, on which
 *                    the radial class is not run)
 *   info[2], [3]     the centre's x, y
 *   seconds[0..3]    contour, shape moments, intensity moments, radial (wall, one thread)
 */
#include <chrono>
#include <cstring>
#include <vector>
#include <unordered_map>
#include <algorithm>

#include "roi_cache.h"
#include "dataset.h"
#include "parallel.h"
#include "features/contour.h"
#include "features/2d_geomoments.h"
#include "features/radial_distribution.h"

using namespace Nyxus;

extern "C" int wsref_slide(const uint32_t* pix, uint32_t w, uint32_t h, double* out, double* info, double* seconds)
{
    if (!pix || !out || !info || w == 0 || h == 0)
        return 1;
    try {
        Fsettings fst;
        fst.resize((int)NyxSetting::__COUNT__);
        fst[(int)NyxSetting::SOFTNAN].rval = 0.0;
        fst[(int)NyxSetting::TINY].rval = 1e-10;
        fst[(int)NyxSetting::SINGLEROI].bval = true;
        fst[(int)NyxSetting::GREYDEPTH].ival = 64;
        fst[(int)NyxSetting::PIXELSIZEUM].rval = 1.0;
        fst[(int)NyxSetting::PIXELDISTANCE].ival = 5;
        fst[(int)NyxSetting::USEGPU].bval = false;
        fst[(int)NyxSetting::VERBOSLVL].ival = 0;
        fst[(int)NyxSetting::IBSI].bval = false;
        Dataset ds;
        std::vector<int> L{1};
        std::unordered_map<int, LR> roiData;
        LR& lr = roiData[1];
        lr.label = 1;
        const size_t n = (size_t)w * h;
        lr.raw_pixels.reserve(n);
        uint32_t mn = pix[0], mx = pix[0];
        for (size_t i = 0; i < n; i++) {
            lr.raw_pixels.push_back(Pixel2((StatsInt)(i % w), (StatsInt)(i / w), (PixIntens)pix[i]));
            mn = std::min(mn, pix[i]); mx = std::max(mx, pix[i]);
        }
        lr.aux_area = (unsigned int)n;
        lr.aux_min = mn;
        lr.aux_max = mx;
        lr.ph_aabb.init_x(0); lr.ph_aabb.update_x((StatsInt)w - 1);
        lr.ph_aabb.init_y(0); lr.ph_aabb.update_y((StatsInt)h - 1);
        lr.make_nonanisotropic_aabb();
        lr.slide_idx = -1;
        lr.initialize_fvals();
        auto t0 = std::chrono::steady_clock::now();
        runParallel(ContourFeature::reduce, 1, 1, 1, &L, &roiData, fst, ds);
        auto t1 = std::chrono::steady_clock::now();
        runParallel(Smoms2D_feature::parallel_process_1_batch, 1, 1, 1, &L, &roiData, fst, ds);
        auto t2 = std::chrono::steady_clock::now();
        runParallel(Imoms2D_feature::parallel_process_1_batch, 1, 1, 1, &L, &roiData, fst, ds);
        auto t3 = std::chrono::steady_clock::now();
        // a 1 x 1 slide has max_sqdist == 0: the class divides by zero and indexes its bins with a converted NaN -- not run
        if (n > 1)
            runParallel(RadialDistributionFeature::parallel_process_1_batch, 1, 1, 1, &L, &roiData, fst, ds);
        auto t4 = std::chrono::steady_clock::now();
        if (seconds) {
            seconds[0] = std::chrono::duration<double>(t1 - t0).count();
            seconds[1] = std::chrono::duration<double>(t2 - t1).count();
            seconds[2] = std::chrono::duration<double>(t3 - t2).count();
            seconds[3] = std::chrono::duration<double>(t4 - t3).count();
        }
        double* p = out;
        for (int f = (int)Feature2D::PERIMETER; f <= (int)Feature2D::EDGE_INTEGRATED_INTENSITY; f++) *p++ = lr.fvals[f][0];
        if (p - out != 7) return 3;
        for (int f = (int)Feature2D::SPAT_MOMENT_00; f <= (int)Feature2D::WEIGHTED_HU_M7; f++) *p++ = lr.fvals[f][0];
        for (int f = (int)Feature2D::IMOM_RM_00; f <= (int)Feature2D::IMOM_WHU7; f++) *p++ = lr.fvals[f][0];
        if (p - out != 187) return 4;
        const Feature2D codes[3] = {Feature2D::FRAC_AT_D, Feature2D::MEAN_FRAC, Feature2D::RADIAL_CV};
        for (int c = 0; c < 3; c++) {
            const std::vector<double>& v = lr.fvals[(int)codes[c]];
            for (int i = 0; i < 8; i++) *p++ = i < (int)v.size() ? v[i] : 0.0;
        }
        std::vector<Pixel2> K;
        lr.merge_multicontour(K);
        if (K.size() != 4) return 5;
        // the identity the sweep kernel relies on: min of the four dist_to_segment == min(x, w-1-x, y, h-1-y), exactly
        double bad = 0;
        for (const Pixel2& q : lr.raw_pixels) {
            if (q.aligned(K[0]) || q.aligned(K[1]) || q.aligned(K[2]) || q.aligned(K[3])) continue;
            const double d = std::min(std::min(q.dist_to_segment(K[0], K[1]), q.dist_to_segment(K[1], K[2])),
                                      std::min(q.dist_to_segment(K[2], K[3]), q.dist_to_segment(K[3], K[0])));
            const long e = std::min(std::min((long)q.x, (long)w - 1 - (long)q.x), std::min((long)q.y, (long)h - 1 - (long)q.y));
            if (d != (double)e) bad += 1;
        }
        info[0] = bad;
        const int c = Pixel2::find_center(lr.raw_pixels, K);
        info[1] = lr.raw_pixels[c].max_sqdist(K);
        info[2] = (double)lr.raw_pixels[c].x;
        info[3] = (double)lr.raw_pixels[c].y;
    } catch (const std::exception& e) {
        fprintf(stderr, "wsref_slide: %s\n", e.what());
        return 2;
    }
    return 0;
}
