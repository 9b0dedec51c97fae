/*
 * ref_morph_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp and tests/golden/circle/ref_circle_driver.cpp) around the
 * reference's own BasicMorphologyFeatures, ContourFeature, ConvexHullFeature and ExtremaFeature classes.  make_morph_golden.py
 * compiles it OUTSIDE the repository against the reference sources where they lie and records what it returns into the fixtures
 * next to this file; nothing compiled from it is kept.
 *
 * Per ROI of a host nyxhip_batch placed at (origin_x[r], origin_y[r]): an LR with ABSOLUTE pixel coordinates in the batch's cloud
 * order, the feature settings filled as compile_feature_settings fills them (env_features.cpp:712-736: the XY resolution slot is
 * never written), and the four classes through their batch reducers in the order of reduce_trivial_2d
 * (reduce_trivial_rois.cpp:83-131):
 *   out[r * 41 ..]   the 41 values in enum order (AREA_PIXELS_COUNT .. ASPECT_RATIO, PERIMETER .. EDGE_INTEGRATED_INTENSITY,
 *                    CIRCULARITY, CONVEX_HULL_AREA, SOLIDITY, EXTREMA_P1_X .. EXTREMA_P8_Y), RAW: +inf stays +inf
 *   n_contour[r]     points of the merged multicontour
 * seconds[0 .. 4): the four classes (wall, n_threads workers), when seconds != NULL.
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
#include "features/convex_hull.h"
#include "features/extrema.h"

#include "nyxhip.h"

using namespace Nyxus;

namespace Nyxus {
void parallelReduceConvHull(size_t start, size_t end, std::vector<int>* ptrLabels, std::unordered_map<int, LR>* ptrLabelData, const Fsettings& s, const Dataset& _);
}

extern "C" int morphref_batch(const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y, double soft_nan, int n_threads,
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
        }
        size_t jobSize = L.size(), workPerThread = jobSize / (size_t)n_threads;
        auto a0 = std::chrono::steady_clock::now();
        runParallel(BasicMorphologyFeatures::parallel_process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto a1 = std::chrono::steady_clock::now();
        runParallel(ContourFeature::reduce, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto a2 = std::chrono::steady_clock::now();
        runParallel(parallelReduceConvHull, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto a3 = std::chrono::steady_clock::now();
        runParallel(ExtremaFeature::reduce, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto a4 = std::chrono::steady_clock::now();
        if (seconds) {
            seconds[0] = std::chrono::duration<double>(a1 - a0).count();
            seconds[1] = std::chrono::duration<double>(a2 - a1).count();
            seconds[2] = std::chrono::duration<double>(a3 - a2).count();
            seconds[3] = std::chrono::duration<double>(a4 - a3).count();
        }
        static const Feature2D codes[41] = {
            Feature2D::AREA_PIXELS_COUNT, Feature2D::AREA_UM2, Feature2D::CENTROID_X, Feature2D::CENTROID_Y, Feature2D::WEIGHTED_CENTROID_Y,
            Feature2D::WEIGHTED_CENTROID_X, Feature2D::MASS_DISPLACEMENT, Feature2D::COMPACTNESS, Feature2D::BBOX_YMIN, Feature2D::BBOX_XMIN,
            Feature2D::BBOX_HEIGHT, Feature2D::BBOX_WIDTH, Feature2D::DIAMETER_EQUAL_AREA, Feature2D::EXTENT, Feature2D::ASPECT_RATIO,
            Feature2D::PERIMETER, Feature2D::DIAMETER_EQUAL_PERIMETER, Feature2D::EDGE_MEAN_INTENSITY, Feature2D::EDGE_STDDEV_INTENSITY,
            Feature2D::EDGE_MAX_INTENSITY, Feature2D::EDGE_MIN_INTENSITY, Feature2D::EDGE_INTEGRATED_INTENSITY,
            Feature2D::CIRCULARITY, Feature2D::CONVEX_HULL_AREA, Feature2D::SOLIDITY,
            Feature2D::EXTREMA_P1_X, Feature2D::EXTREMA_P1_Y, Feature2D::EXTREMA_P2_X, Feature2D::EXTREMA_P2_Y, Feature2D::EXTREMA_P3_X,
            Feature2D::EXTREMA_P3_Y, Feature2D::EXTREMA_P4_X, Feature2D::EXTREMA_P4_Y, Feature2D::EXTREMA_P5_X, Feature2D::EXTREMA_P5_Y,
            Feature2D::EXTREMA_P6_X, Feature2D::EXTREMA_P6_Y, Feature2D::EXTREMA_P7_X, Feature2D::EXTREMA_P7_Y, Feature2D::EXTREMA_P8_X,
            Feature2D::EXTREMA_P8_Y};
        for (uint64_t r = 0; r < b->n_roi; r++) {
            LR& lr = roiData[(int)r + 1];
            if (n_contour) {
                std::vector<Pixel2> K;
                lr.merge_multicontour(K);
                n_contour[r] = (int32_t)K.size();
            }
            double* o = out + r * 41;
            for (int i = 0; i < 41; i++)
                o[i] = lr.fvals[(int)codes[i]][0];
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "morphref_batch: %s\n", e.what());
        return 2;
    }
    return 0;
}
