/*
 * ref_radial_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp) around the reference's own ContourFeature and
 * RadialDistributionFeature classes.  make_radial_golden.py compiles it OUTSIDE the repository against the reference
 * sources where they lie and records what it returns into the fixtures next to this file; nothing compiled from it is kept.
 *
 * Per ROI of a host nyxhip_batch: LR exactly as oracle/ref_driver.cpp builds it (box origin 0), the ladder
 * ContourFeature::reduce -> RadialDistributionFeature::parallel_process_1_batch (reduce_trivial_rois.cpp), then
 *   out[r * 24 ..]   FRAC_AT_D[8] | MEAN_FRAC[8] | RADIAL_CV[8]   (LR::fvals)
 *   dst2[r]          max_sqdist of the centre pixel over the merged contour (dstOC^2; 0 = the reference's undefined case;
 *                    -1 = no contour)
 *   n_contour[r]     points of the merged multicontour
 * seconds[0] = contour ladder, seconds[1] = radial ladder (wall, n_threads workers).
 */
#include <chrono>
#include <cstring>
#include <vector>
#include <unordered_map>

#include "roi_cache.h"
#include "dataset.h"
#include "parallel.h"
#include "features/contour.h"
#include "features/radial_distribution.h"

#include "nyxhip.h"

using namespace Nyxus;

extern "C" int radref_batch(const nyxhip_batch* b, int n_threads, double* out, double* dst2, int32_t* n_contour, double* seconds)
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
        runParallel(RadialDistributionFeature::parallel_process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto t2 = std::chrono::steady_clock::now();
        if (seconds) {
            seconds[0] = std::chrono::duration<double>(t1 - t0).count();
            seconds[1] = std::chrono::duration<double>(t2 - t1).count();
        }
        for (uint64_t r = 0; r < b->n_roi; r++) {
            LR& lr = roiData[(int)r + 1];
            const Feature2D codes[3] = {Feature2D::FRAC_AT_D, Feature2D::MEAN_FRAC, Feature2D::RADIAL_CV};
            for (int c = 0; c < 3; c++) {
                const std::vector<double>& v = lr.fvals[(int)codes[c]];
                for (int i = 0; i < 8; i++) out[r * 24 + c * 8 + i] = i < (int)v.size() ? v[i] : 0.0;
            }
            std::vector<Pixel2> K;
            lr.merge_multicontour(K);
            if (n_contour) n_contour[r] = (int32_t)K.size();
            if (dst2) {
                if (K.empty() || lr.raw_pixels.empty())
                    dst2[r] = -1.0;
                else
                    dst2[r] = lr.raw_pixels[Pixel2::find_center(lr.raw_pixels, K)].max_sqdist(K);
            }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "radref_batch: %s\n", e.what());
        return 2;
    }
    return 0;
}
