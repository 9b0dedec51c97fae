/*
 * ref_caliper_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp and tests/golden/outline/ref_outline_driver.cpp) around the
 * reference's own ConvexHullFeature, CaliperFeretFeature, CaliperMartinFeature and CaliperNassensteinFeature classes.
 * make_caliper_golden.py compiles it OUTSIDE the repository against the reference sources where they lie and records what it
 * returns into the fixtures next to this file; nothing compiled from it is kept.
 *
 * Per ROI of a host nyxhip_batch placed at (origin_x[r], origin_y[r]): an LR with ABSOLUTE pixel coordinates,
 * ConvexHullFeature::calculate (which runs build_convex_hull into LR::convHull_CH), then the three classes' extract():
 *   out[r * 20 ..]      the 20 columns in enum order (featureset.h:93-114)
 *   hull_n[r]           vertices of the hull; hull_xy: their coordinates RELATIVE to the origin, x y pairs, ROI after ROI
 *                       (hull_cap pairs at most; the call fails beyond)
 *   per_angle[r * 57 ..] the per-angle diameters the classes' own (private) measurement loops return: 19 Feret, 19 Martin,
 *                       19 Nassenstein slots in angle order, NaN-padded (the loops drop skipped angles, so slot j is the j-th KEPT
 *                       value; Feret's angles go to feret_angle[r * 19 ..])
 * seconds[0..3] = hull, Feret, Martin, Nassenstein ladders (wall, n_threads workers), when seconds != NULL.
 */
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include <unordered_map>

#include "roi_cache.h"
#include "dataset.h"
#include "parallel.h"
#include "helpers/helpers.h"
#include "features/convex_hull.h"
#define private public                      /* the measurement loops (calculate_imp, calculate_angled_caliper_measurements) */
#include "features/caliper.h"
#undef private

#include "nyxhip.h"

using namespace Nyxus;

extern "C" int calref_batch(const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y, double soft_nan, int n_threads,
                            double* out, int32_t* hull_n, int32_t* hull_xy, int64_t hull_cap, double* per_angle, double* feret_angle,
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
        if (seconds) {
            auto a0 = std::chrono::steady_clock::now();
            runParallel(parallelReduceConvHull, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
            auto a1 = std::chrono::steady_clock::now();
            runParallel(CaliperFeretFeature::parallel_process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
            auto a2 = std::chrono::steady_clock::now();
            runParallel(CaliperMartinFeature::parallel_process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
            auto a3 = std::chrono::steady_clock::now();
            runParallel(CaliperNassensteinFeature::parallel_process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
            auto a4 = std::chrono::steady_clock::now();
            seconds[0] = std::chrono::duration<double>(a1 - a0).count();
            seconds[1] = std::chrono::duration<double>(a2 - a1).count();
            seconds[2] = std::chrono::duration<double>(a3 - a2).count();
            seconds[3] = std::chrono::duration<double>(a4 - a3).count();
        }
        const double nan = std::numeric_limits<double>::quiet_NaN();
        int64_t hull_used = 0;
        for (uint64_t r = 0; r < b->n_roi; r++) {
            LR& lr = roiData[(int)r + 1];
            const StatsInt ox = origin_x ? (StatsInt)origin_x[r] : 0, oy = origin_y ? (StatsInt)origin_y[r] : 0;
            ConvexHullFeature::extract(lr, fst);
            CaliperFeretFeature::extract(lr, fst);
            CaliperMartinFeature::extract(lr, fst);
            CaliperNassensteinFeature::extract(lr, fst);
            double* o = out + r * 20;
            for (int i = 0; i < 8; i++) o[i] = lr.fvals[(int)Feature2D::MIN_FERET_ANGLE + i][0];
            for (int i = 0; i < 6; i++) o[8 + i] = lr.fvals[(int)Feature2D::STAT_MARTIN_DIAM_MIN + i][0];
            for (int i = 0; i < 6; i++) o[14 + i] = lr.fvals[(int)Feature2D::STAT_NASSENSTEIN_DIAM_MIN + i][0];
            if (hull_n) {
                hull_n[r] = (int32_t)lr.convHull_CH.size();
                if (hull_used + (int64_t)lr.convHull_CH.size() > hull_cap) return 3;
                for (const Pixel2& p : lr.convHull_CH) {
                    hull_xy[2 * hull_used] = (int32_t)(p.x - ox); hull_xy[2 * hull_used + 1] = (int32_t)(p.y - oy);
                    hull_used++;
                }
            }
            if (per_angle) {
                double* pa = per_angle + r * 57;
                for (int i = 0; i < 57; i++) pa[i] = nan;
                for (int i = 0; i < 19; i++) feret_angle[r * 19 + i] = nan;
                if (lr.convHull_CH.size()) {
                    std::vector<float> ang;
                    std::vector<double> fe, ma, na;
                    CaliperFeretFeature ff; ff.calculate_angled_caliper_measurements(lr.convHull_CH, ang, fe);
                    CaliperMartinFeature mf; mf.calculate_imp(lr.convHull_CH, ma);
                    CaliperNassensteinFeature nf; nf.calculate_imp(lr.convHull_CH, na);
                    for (size_t i = 0; i < fe.size() && i < 19; i++) { pa[i] = fe[i]; feret_angle[r * 19 + i] = ang[i]; }
                    for (size_t i = 0; i < ma.size() && i < 19; i++) pa[19 + i] = ma[i];
                    for (size_t i = 0; i < na.size() && i < 19; i++) pa[38 + i] = na[i];
                }
            }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "calref_batch: %s\n", e.what());
        return 2;
    }
    return 0;
}
