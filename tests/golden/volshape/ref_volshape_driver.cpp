/*
 * ref_volshape_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of tests/golden/voldzone/ref_voldzone_driver.cpp) around the reference's own D3_SurfaceFeature
 * class.  make_volshape_golden.py compiles it OUTSIDE the repository against the reference sources where they lie and records what it
 * returns into the fixtures next to this file; nothing compiled from it is kept.
 *
 * Per ROI of a host nyxhip_batch3d: an LR with the batch's voxel cloud in BOX-RELATIVE coordinates, the z-plane index lists the
 * reference's pixel feed keeps (LR::zplanes) and its box; the class's calculate + save_value through its reduce(), with an Fsettings
 * that holds soft_nan and single-ROI mode off.
 *   out[r * 14 ..]  the 14 codes AREA .. FLATNESS as the class leaves them (NaN / inf NOT replaced)
 * An ROI without voxels is refused (return 4).  seconds[0] = the runParallel() call (wall, n_threads workers), when seconds != NULL.
 */
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>
#include <unordered_map>

#include "roi_cache.h"
#include "dataset.h"
#include "parallel.h"
#include "features/3d_surface.h"

#include "nyxhip.h"

using namespace Nyxus;

static const int N_COL = 14;

extern "C" int volshaperef_batch(const nyxhip_batch3d* b, const nyxhip_settings* s, int n_threads, double* out, double* seconds)
{
    if (!b || !s || !out || b->memory != NYXHIP_MEM_HOST || n_threads < 1)
        return 1;
    for (uint64_t r = 0; r < b->n_roi; r++)
        if (b->px_offset[r + 1] == b->px_offset[r])
            return 4;
    try {
        Fsettings fst;
        fst.resize((int)NyxSetting::__COUNT__);
        fst[(int)NyxSetting::SOFTNAN].rval = s->soft_nan;
        fst[(int)NyxSetting::TINY].rval = 0.0;
        fst[(int)NyxSetting::SINGLEROI].bval = false;
        fst[(int)NyxSetting::GREYDEPTH].ival = s->grey_depth;
        fst[(int)NyxSetting::PIXELSIZEUM].rval = 100;
        fst[(int)NyxSetting::PIXELDISTANCE].ival = 5;
        fst[(int)NyxSetting::USEGPU].bval = false;
        fst[(int)NyxSetting::VERBOSLVL].ival = 0;
        fst[(int)NyxSetting::IBSI].bval = s->ibsi != 0;
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
            lr.raw_pixels_3D.reserve(n);
            for (uint64_t i = 0; i < n; i++) {
                lr.raw_pixels_3D.push_back(Pixel3((StatsInt)b->x[o + i], (StatsInt)b->y[o + i], (StatsInt)b->z[o + i], (PixIntens)b->inten[o + i]));
                lr.zplanes[(int)b->z[o + i]].push_back((size_t)i);
            }
            lr.aux_area = (unsigned int)n;
            lr.aux_min = b->min_inten[r];
            lr.aux_max = b->max_inten[r];
            lr.ph_aabb.init_x(0); lr.ph_aabb.update_x((StatsInt)b->bbox_w[r] - 1);
            lr.ph_aabb.init_y(0); lr.ph_aabb.update_y((StatsInt)b->bbox_h[r] - 1);
            lr.ph_aabb.init_z(0); lr.ph_aabb.update_z((StatsInt)b->bbox_d[r] - 1);
            lr.make_nonanisotropic_aabb();
            lr.slide_idx = -1;
            lr.initialize_fvals();
        }
        size_t jobSize = L.size(), workPerThread = jobSize / (size_t)n_threads;
        auto a0 = std::chrono::steady_clock::now();
        runParallel(D3_SurfaceFeature::reduce, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto a1 = std::chrono::steady_clock::now();
        if (seconds)
            seconds[0] = std::chrono::duration<double>(a1 - a0).count();
        for (uint64_t r = 0; r < b->n_roi; r++) {
            LR& lr = roiData[(int)r + 1];
            for (int i = 0; i < N_COL; i++)
                out[r * N_COL + i] = lr.fvals[(int)Feature3D::AREA + i][0];
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "volshaperef_batch: %s\n", e.what());
        return 2;
    }
    return 0;
}
