/*
 * ref_outline_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp and tests/golden/radial/ref_radial_driver.cpp) around the
 * reference's own ContourFeature, FractalDimensionFeature, EulerNumberFeature and RoiRadiusFeature classes.
 * make_outline_golden.py compiles it OUTSIDE the repository against the reference sources where they lie and records what it
 * returns into the fixtures next to this file; nothing compiled from it is kept.
 *
 * Per ROI of a host nyxhip_batch: LR exactly as oracle/ref_driver.cpp builds it (box origin 0), ContourFeature::reduce, then the
 * three classes' extract():
 *   out[r * 6 ..]        FRACT_DIM_BOXCOUNT, FRACT_DIM_PERIMETER, EULER_NUMBER, ROI_RADIUS_MEAN, ROI_RADIUS_MAX, ROI_RADIUS_MEDIAN
 *   n_contour[r]         points of the merged multicontour
 *   box_counts[r*20 ..]  ROIs whose padded side is <= 32: per box size 32, 16, 8, 4, 2 the pixel-occupied boxes of the four grid
 *                        origins (0,0), (s/2,0), (0,s/2), (s/2,s/2) -- counted here from the LR's own pixels and box; -1 where the
 *                        size exceeds the padded side or the ROI takes the single-grid path
 * RoiRadiusFeature is NOT run on an ROI whose merged contour is one point: Pixel2::min_sqdist converts 1 / log(1) to int there
 * (undefined); its three values come back as NaN and the generator refuses to compare them.
 * seconds[0] = contour ladder, seconds[1..3] = fractal, Euler, radius ladders (wall, n_threads workers; timed only when every
 * contour has != 1 points).
 */
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <set>
#include <vector>
#include <unordered_map>

#include "roi_cache.h"
#include "dataset.h"
#include "parallel.h"
#include "helpers/helpers.h"
#include "features/contour.h"
#include "features/fractal_dim.h"
#include "features/euler_number.h"
#include "features/roi_radius.h"

#include "nyxhip.h"

using namespace Nyxus;

extern "C" int outref_batch(const nyxhip_batch* b, int n_threads, double* out, int32_t* n_contour, int32_t* box_counts, double* seconds)
{
    if (!b || !out || b->memory != NYXHIP_MEM_HOST || n_threads < 1)
        return 1;
    try {
        Fsettings fst;
        fst.resize((int)NyxSetting::__COUNT__);
        fst[(int)NyxSetting::SOFTNAN].rval = 0.0;
        fst[(int)NyxSetting::TINY].rval = 1e-10;
        fst[(int)NyxSetting::SINGLEROI].bval = false;
        fst[(int)NyxSetting::GREYDEPTH].ival = 64;
        fst[(int)NyxSetting::PIXELSIZEUM].rval = 1.0;
        fst[(int)NyxSetting::PIXELDISTANCE].ival = 5;
        fst[(int)NyxSetting::USEGPU].bval = false;
        fst[(int)NyxSetting::VERBOSLVL].ival = 0;
        fst[(int)NyxSetting::IBSI].bval = false;
        Dataset ds;
        std::vector<int> L;
        std::unordered_map<int, LR> roiData;
        L.reserve(b->n_roi);
        roiData.reserve(b->n_roi);
        for (uint64_t r = 0; r < b->n_roi; r++) {
            int lab = (int)r + 1;
            L.push_back(lab);
            LR& lr = roiData[lab];
            lr.label = lab;
            uint64_t o = b->px_offset[r], n = b->px_offset[r + 1] - o;
            lr.raw_pixels.reserve(n);
            for (uint64_t i = 0; i < n; i++)
                lr.raw_pixels.push_back(Pixel2((StatsInt)b->x[o + i], (StatsInt)b->y[o + i], (PixIntens)b->inten[o + i]));
            lr.aux_area = (unsigned int)n;
            lr.aux_min = b->min_inten[r];
            lr.aux_max = b->max_inten[r];
            lr.ph_aabb.init_x(0); lr.ph_aabb.update_x((StatsInt)b->bbox_w[r] - 1);
            lr.ph_aabb.init_y(0); lr.ph_aabb.update_y((StatsInt)b->bbox_h[r] - 1);
            lr.make_nonanisotropic_aabb();
            lr.slide_idx = -1;
            lr.aux_image_matrix.allocate((int)b->bbox_w[r], (int)b->bbox_h[r]);
            lr.aux_image_matrix.calculate_from_pixelcloud(lr.raw_pixels, lr.aabb);
            lr.initialize_fvals();
        }
        size_t jobSize = L.size(), workPerThread = jobSize / (size_t)n_threads;
        auto t0 = std::chrono::steady_clock::now();
        runParallel(ContourFeature::reduce, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto t1 = std::chrono::steady_clock::now();
        if (seconds) seconds[0] = std::chrono::duration<double>(t1 - t0).count();
        bool all_defined = true;
        for (uint64_t r = 0; r < b->n_roi; r++) {
            std::vector<Pixel2> K;
            roiData[(int)r + 1].merge_multicontour(K);
            if (n_contour) n_contour[r] = (int32_t)K.size();
            if (K.size() == 1) all_defined = false;
        }
        const double nan = std::numeric_limits<double>::quiet_NaN();
        if (seconds && all_defined) {
            auto a0 = std::chrono::steady_clock::now();
            runParallel(FractalDimensionFeature::parallel_process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
            auto a1 = std::chrono::steady_clock::now();
            runParallel(EulerNumberFeature::reduce, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
            auto a2 = std::chrono::steady_clock::now();
            runParallel(RoiRadiusFeature::parallel_process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
            auto a3 = std::chrono::steady_clock::now();
            seconds[1] = std::chrono::duration<double>(a1 - a0).count();
            seconds[2] = std::chrono::duration<double>(a2 - a1).count();
            seconds[3] = std::chrono::duration<double>(a3 - a2).count();
        }
        for (uint64_t r = 0; r < b->n_roi; r++) {
            LR& lr = roiData[(int)r + 1];
            std::vector<Pixel2> K;
            lr.merge_multicontour(K);
            FractalDimensionFeature::extract(lr, fst);
            EulerNumberFeature::extract(lr, fst);
            const bool radius_defined = K.size() != 1;
            if (radius_defined) RoiRadiusFeature::extract(lr, fst);
            double* o = out + r * 6;
            o[0] = lr.fvals[(int)Feature2D::FRACT_DIM_BOXCOUNT][0];
            o[1] = lr.fvals[(int)Feature2D::FRACT_DIM_PERIMETER][0];
            o[2] = lr.fvals[(int)Feature2D::EULER_NUMBER][0];
            o[3] = radius_defined ? lr.fvals[(int)Feature2D::ROI_RADIUS_MEAN][0] : nan;
            o[4] = radius_defined ? lr.fvals[(int)Feature2D::ROI_RADIUS_MAX][0] : nan;
            o[5] = radius_defined ? lr.fvals[(int)Feature2D::ROI_RADIUS_MEDIAN][0] : nan;
            if (box_counts) {
                int32_t* bc = box_counts + r * 20;
                for (int i = 0; i < 20; i++) bc[i] = -1;
                const int side = Nyxus::ceil_pow2((int)std::max(lr.aabb.get_width(), lr.aabb.get_height()));
                if (side <= 32 && lr.raw_pixels.size() >= 2)
                    for (int s = 32, row = 0; s > 1; s >>= 1, row++) {
                        if (s > side) continue;
                        for (int og = 0; og < 4; og++) {
                            const int ox = (og & 1) * s / 2, oy = (og >> 1) * s / 2;
                            std::set<std::pair<int, int>> boxes;
                            for (const Pixel2& p : lr.raw_pixels)
                                boxes.insert({(int)(p.y - lr.aabb.get_ymin() + oy) / s, (int)(p.x - lr.aabb.get_xmin() + ox) / s});
                            bc[row * 4 + og] = (int32_t)boxes.size();
                        }
                    }
            }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "outref_batch: %s\n", e.what());
        return 2;
    }
    return 0;
}
