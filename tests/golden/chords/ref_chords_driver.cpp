/*
 * ref_chords_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp and tests/golden/caliper/ref_caliper_driver.cpp) around the
 * reference's own ChordsFeature class.  make_chords_golden.py compiles it OUTSIDE the repository against the reference sources
 * where they lie and records what it returns into the fixtures next to this file; nothing compiled from it is kept.
 *
 * Per ROI of a host nyxhip_batch placed at (origin_x[r], origin_y[r]): an LR with ABSOLUTE pixel coordinates in the batch's cloud
 * order, then ChordsFeature::extract():
 *   out[r * 16 ..]        the 16 columns in enum order (featureset.h:117-132), each passed through the output stage's
 *                         "not finite -> soft_nan" replacement (output_2_buffer.cpp)
 *   per_angle[r * 60 ..]  what the class's angle loop sees, taken with the reference's own Rotation::rotate_cloud, ImageMatrix and
 *                         ImageMatrix::get_chlen in the loop of chords.cpp:23-47: 20 per-angle maxima (0: no chord), 20 counts of
 *                         chords > 0, 20 sums of them
 * seconds[0] = the ChordsFeature ladder (wall, n_threads workers), when seconds != NULL.
 */
#define _USE_MATH_DEFINES
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
#include "features/chords.h"
#include "features/image_matrix.h"
#include "features/rotation.h"

#include "nyxhip.h"

using namespace Nyxus;

extern "C" int chordsref_batch(const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y, double soft_nan, int n_threads,
                               double* out, int64_t* per_angle, double* seconds)
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
        if (seconds) {
            size_t jobSize = L.size(), workPerThread = jobSize / (size_t)n_threads;
            auto a0 = std::chrono::steady_clock::now();
            runParallel(ChordsFeature::process_1_batch, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
            auto a1 = std::chrono::steady_clock::now();
            seconds[0] = std::chrono::duration<double>(a1 - a0).count();
        }
        for (uint64_t r = 0; r < b->n_roi; r++) {
            LR& lr = roiData[(int)r + 1];
            ChordsFeature::extract(lr, fst);
            double* o = out + r * 16;
            for (int i = 0; i < 16; i++) {
                const double v = lr.fvals[(int)Feature2D::MAXCHORDS_MAX + i][0];
                o[i] = std::isfinite(v) ? v : soft_nan;
            }
            if (per_angle) {
                int64_t* pa = per_angle + r * 60;
                memset(pa, 0, 60 * sizeof(int64_t));
                const double cenx = (lr.aabb.get_xmin() + lr.aabb.get_xmax()) / 2.0, ceny = (lr.aabb.get_ymin() + lr.aabb.get_ymax()) / 2.0;
                const double angStep = M_PI / 20.0;
                int k = 0;
                for (double ang = 0; ang < M_PI; ang += angStep, k++) {
                    if (k >= 20) return 4;
                    std::vector<Pixel2> R;
                    R.resize(lr.raw_pixels.size(), {0, 0, 0});
                    Rotation::rotate_cloud(lr.raw_pixels, cenx, ceny, ang, R);
                    ImageMatrix im(R);
                    const int step = im.width >= 200 ? im.width / 100 : 1;
                    for (int col = 0; col < im.width; col += step) {
                        const int c = im.get_chlen(col);
                        if (c > 0) { pa[k] = std::max<int64_t>(pa[k], c); pa[20 + k]++; pa[40 + k] += c; }
                    }
                }
                if (k != 20) return 5;
            }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "chordsref_batch: %s\n", e.what());
        return 2;
    }
    return 0;
}
