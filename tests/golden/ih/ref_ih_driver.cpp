/*
 * ref_ih_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp and tests/golden/circle/ref_circle_driver.cpp) around the reference's
 * own IntensityHistogramFeatures class.  make_ih_golden.py compiles it OUTSIDE the repository against the reference sources where they
 * lie and records what it returns into the fixtures next to this file; nothing compiled from it is kept.
 *
 * Per ROI of a host nyxhip_batch: an LR with the batch's pixel cloud, aux_min / aux_max from the batch, slide_idx = -1 (an integer image:
 * float_domain_map is the identity); the class through its reduce():
 *   out[r * 46 ..]      IH_MEAN_VAL .. IH_BIN_SIZE (enum order), as the class leaves them (NaN / inf are NOT replaced)
 *   counts[r * N ..]    the N bin counts, by the class's own binning expression evaluated here (the class keeps its histogram in a local);
 *                       zeros for an ROI the class gates.  counts may be NULL.
 * seconds[0] = the class's reduce (wall, n_threads workers), when seconds != NULL.
 */
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>
#include <unordered_map>

#include "roi_cache.h"
#include "dataset.h"
#include "parallel.h"
#include "features/intensity_histogram.h"

#include "nyxhip.h"

using namespace Nyxus;

extern "C" int ihref_batch(const nyxhip_batch* b, int grey_depth, int ibsi, double soft_nan, int n_threads, double* out, uint64_t* counts,
                           double* seconds)
{
    if (!b || !out || b->memory != NYXHIP_MEM_HOST || n_threads < 1)
        return 1;
    try {
        Fsettings fst;
        fst.resize((int)NyxSetting::__COUNT__);
        fst[(int)NyxSetting::SOFTNAN].rval = soft_nan;
        fst[(int)NyxSetting::TINY].rval = 1e-10;
        fst[(int)NyxSetting::SINGLEROI].bval = false;
        fst[(int)NyxSetting::GREYDEPTH].ival = grey_depth;
        fst[(int)NyxSetting::PIXELSIZEUM].rval = 1.0;
        fst[(int)NyxSetting::PIXELDISTANCE].ival = 5;
        fst[(int)NyxSetting::XYRES].rval = 0.0;
        fst[(int)NyxSetting::USEGPU].bval = false;
        fst[(int)NyxSetting::VERBOSLVL].ival = 0;
        fst[(int)NyxSetting::IBSI].bval = ibsi != 0;
        fst[(int)NyxSetting::FPIMG_ACTIVE].bval = false;
        fst[(int)NyxSetting::FPIMG_MIN].rval = 0.0;
        fst[(int)NyxSetting::FPIMG_MAX].rval = 1.0;
        fst[(int)NyxSetting::FPIMG_TARGET_DR].rval = 1e4;
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
            lr.slide_idx = -1;
            lr.initialize_fvals();
        }
        size_t jobSize = L.size(), workPerThread = jobSize / (size_t)n_threads;
        auto a0 = std::chrono::steady_clock::now();
        runParallel(IntensityHistogramFeatures::reduce, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto a1 = std::chrono::steady_clock::now();
        if (seconds)
            seconds[0] = std::chrono::duration<double>(a1 - a0).count();
        const int first = (int)Feature2D::IH_MEAN_VAL;
        if ((int)Feature2D::IH_BIN_SIZE - first != 45)
            return 3;
        for (uint64_t r = 0; r < b->n_roi; r++) {
            LR& lr = roiData[(int)r + 1];
            for (int i = 0; i < 46; i++)
                out[r * 46 + i] = lr.fvals[first + i][0];
            if (counts && grey_depth >= 2) {
                const int N = grey_depth;
                uint64_t* c = counts + r * (uint64_t)N;
                memset(c, 0, sizeof(uint64_t) * (size_t)N);
                const double mn = lr.aux_min, mx = lr.aux_max;
                if (!ibsi || mx <= mn || lr.raw_pixels.empty())
                    continue;
                const double binWidth = (mx - mn) / double(N);
                for (auto& px : lr.raw_pixels) {
                    double v = 0.0 + 1.0 * (double)px.inten;
                    int idx = (int)std::floor((v - mn) / binWidth);
                    if (idx < 0) idx = 0;
                    if (idx >= N) idx = N - 1;
                    c[idx]++;
                }
            }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "ihref_batch: %s\n", e.what());
        return 2;
    }
    return 0;
}
