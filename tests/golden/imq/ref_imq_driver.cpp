/*
 * ref_imq_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp and tests/golden/ih/ref_ih_driver.cpp) around the reference's own
 * FocusScoreFeature and SaturationFeature classes.  make_imq_golden.py compiles it OUTSIDE the repository against the reference sources
 * where they lie and records what it returns into the fixtures next to this file; nothing compiled from it is kept.
 *
 * Per ROI of a host nyxhip_batch: an LR with the batch's pixel cloud, its box and its dense image matrix (LR::aux_image_matrix, built by the
 * reference's own calculate_from_pixelcloud); the two classes through parallel_process_1_batch(), as reduce_trivial_2d runs them:
 *   out[r * 4 ..]   FOCUS_SCORE, LOCAL_FOCUS_SCORE, MAX_SATURATION, MIN_SATURATION as the classes leave them (NaN / inf are NOT replaced)
 * A box with a side of 1 is refused (return 4): the reference's LOCAL_FOCUS_SCORE loop does not end on it.
 * seconds[0] = the two runParallel() calls (wall, n_threads workers), when seconds != NULL.
 */
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>
#include <unordered_map>

#include "roi_cache.h"
#include "dataset.h"
#include "parallel.h"
#include "features/focus_score.h"
#include "features/saturation.h"

#include "nyxhip.h"

using namespace Nyxus;

extern "C" int imqref_batch(const nyxhip_batch* b, double soft_nan, int n_threads, double* out, double* seconds)
{
    if (!b || !out || b->memory != NYXHIP_MEM_HOST || n_threads < 1)
        return 1;
    for (uint64_t r = 0; r < b->n_roi; r++)
        if (b->bbox_w[r] < 2 || b->bbox_h[r] < 2 || b->px_offset[r + 1] == b->px_offset[r])
            return 4;
    try {
        Fsettings fst;
        fst.resize((int)NyxSetting::__COUNT__);
        fst[(int)NyxSetting::SOFTNAN].rval = soft_nan;
        fst[(int)NyxSetting::TINY].rval = 1e-10;
        fst[(int)NyxSetting::SINGLEROI].bval = false;
        fst[(int)NyxSetting::GREYDEPTH].ival = 256;
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
            lr.aux_image_matrix.allocate(lr.aabb.get_width(), lr.aabb.get_height());
            lr.aux_image_matrix.calculate_from_pixelcloud(lr.raw_pixels, lr.aabb);
            lr.initialize_fvals();
        }
        size_t jobSize = L.size(), workPerThread = jobSize / (size_t)n_threads;
        auto a0 = std::chrono::steady_clock::now();
        runParallel(FocusScoreFeature::parallel_process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        runParallel(SaturationFeature::parallel_process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto a1 = std::chrono::steady_clock::now();
        if (seconds)
            seconds[0] = std::chrono::duration<double>(a1 - a0).count();
        static const FeatureIMQ codes[4] = {FeatureIMQ::FOCUS_SCORE, FeatureIMQ::LOCAL_FOCUS_SCORE, FeatureIMQ::MAX_SATURATION, FeatureIMQ::MIN_SATURATION};
        for (uint64_t r = 0; r < b->n_roi; r++) {
            LR& lr = roiData[(int)r + 1];
            for (int i = 0; i < 4; i++)
                out[r * 4 + i] = lr.fvals[(int)codes[i]][0];
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "imqref_batch: %s\n", e.what());
        return 2;
    }
    return 0;
}
