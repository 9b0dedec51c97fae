/*
 * ref_circle_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp and tests/golden/erosion/ref_erosion_driver.cpp) around the
 * reference's own EnclosingInscribingCircumscribingCircleFeature and GeodeticLengthThicknessFeature classes.  make_circle_golden.py
 * compiles it OUTSIDE the repository against the reference sources where they lie and records what it returns into the fixtures
 * next to this file; nothing compiled from it is kept.
 *
 * Per ROI of a host nyxhip_batch placed at (origin_x[r], origin_y[r]): an LR with ABSOLUTE pixel coordinates in the batch's cloud
 * order; BasicMorphologyFeatures (CENTROID_X / _Y), ContourFeature (PERIMETER and LR::multicontour_), then the two classes through
 * their parallel_process_1_batch (the circle class's carries the "empty contour" skip):
 *   out[r * 8 ..]   DIAMETER_MIN_ENCLOSING_CIRCLE, DIAMETER_CIRCUMSCRIBING_CIRCLE, DIAMETER_INSCRIBING_CIRCLE, GEODETIC_LENGTH,
 *                   THICKNESS (enum order), PERIMETER, CENTROID_X, CENTROID_Y, each passed through "not finite -> soft_nan"
 *   n_contour[r]    points of the merged multicontour
 * seconds[0] = the circle class, seconds[1] = the geodetic class (wall, n_threads workers), when seconds != NULL.
 */
#define _USE_MATH_DEFINES
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>
#include <unordered_map>

#include "roi_cache.h"
#include "dataset.h"
#include "parallel.h"
#include "helpers/helpers.h"
#include "features/basic_morphology.h"
#include "features/contour.h"
#include "features/circle.h"
#include "features/geodetic_len_thickness.h"

#include "nyxhip.h"

using namespace Nyxus;

extern "C" int circleref_batch(const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y, double soft_nan, int n_threads,
                               double* out, int32_t* n_contour, double* seconds)
{
    if (!b || !out || b->memory != NYXHIP_MEM_HOST || n_threads < 1)
        return 1;
    try {
        Fsettings fst;
        fst.resize((int)NyxSetting::__COUNT__);
        fst[(int)NyxSetting::SOFTNAN].rval = soft_nan;
        fst[(int)NyxSetting::TINY].rval = 1e-10;
        fst[(int)NyxSetting::SINGLEROI].bval = false;
        fst[(int)NyxSetting::GREYDEPTH].ival = 64;
        fst[(int)NyxSetting::PIXELSIZEUM].rval = 1.0;
        fst[(int)NyxSetting::PIXELDISTANCE].ival = 5;
        fst[(int)NyxSetting::XYRES].rval = 0.0;
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
            const StatsInt ox = origin_x ? (StatsInt)origin_x[r] : 0, oy = origin_y ? (StatsInt)origin_y[r] : 0;
            uint64_t o = b->px_offset[r], n = b->px_offset[r + 1] - o;
            lr.raw_pixels.reserve(n);
            for (uint64_t i = 0; i < n; i++)
                lr.raw_pixels.push_back(Pixel2((StatsInt)b->x[o + i] + ox, (StatsInt)b->y[o + i] + oy, (PixIntens)b->inten[o + i]));
            lr.aux_area = (unsigned int)n;
            lr.aux_min = b->min_inten[r];
            lr.aux_max = b->max_inten[r];
            lr.ph_aabb.init_x(ox); lr.ph_aabb.update_x(ox + (StatsInt)b->bbox_w[r] - 1);
            lr.ph_aabb.init_y(oy); lr.ph_aabb.update_y(oy + (StatsInt)b->bbox_h[r] - 1);
            lr.make_nonanisotropic_aabb();
            lr.slide_idx = -1;
            lr.initialize_fvals();
            BasicMorphologyFeatures bm;
            bm.calculate(lr, fst);
            bm.save_value(lr.fvals);
        }
        size_t jobSize = L.size(), workPerThread = jobSize / (size_t)n_threads;
        runParallel(ContourFeature::reduce, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto a0 = std::chrono::steady_clock::now();
        runParallel(EnclosingInscribingCircumscribingCircleFeature::parallel_process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto a1 = std::chrono::steady_clock::now();
        runParallel(GeodeticLengthThicknessFeature::parallel_process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto a2 = std::chrono::steady_clock::now();
        if (seconds) {
            seconds[0] = std::chrono::duration<double>(a1 - a0).count();
            seconds[1] = std::chrono::duration<double>(a2 - a1).count();
        }
        static const Feature2D codes[8] = {Feature2D::DIAMETER_MIN_ENCLOSING_CIRCLE, Feature2D::DIAMETER_CIRCUMSCRIBING_CIRCLE,
                                           Feature2D::DIAMETER_INSCRIBING_CIRCLE, Feature2D::GEODETIC_LENGTH, Feature2D::THICKNESS,
                                           Feature2D::PERIMETER, Feature2D::CENTROID_X, Feature2D::CENTROID_Y};
        for (uint64_t r = 0; r < b->n_roi; r++) {
            LR& lr = roiData[(int)r + 1];
            if (n_contour) {
                std::vector<Pixel2> K;
                lr.merge_multicontour(K);
                n_contour[r] = (int32_t)K.size();
            }
            double* o = out + r * 8;
            for (int i = 0; i < 8; i++) {
                const double v = lr.fvals[(int)codes[i]][0];
                o[i] = std::isfinite(v) ? v : soft_nan;
            }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "circleref_batch: %s\n", e.what());
        return 2;
    }
    return 0;
}
