/*
 * ref_vol_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp and tests/golden/imq/ref_imq_driver.cpp) around the reference's own
 * D3_VoxelIntensityFeatures and D3_GLCM_feature classes.  make_vol_golden.py compiles it OUTSIDE the repository against the reference
 * sources where they lie and records what it returns into the fixtures next to this file; nothing compiled from it is kept.
 *
 * Per ROI of a host nyxhip_batch3d: an LR with the batch's voxel cloud (raw_pixels_3D), its box, its dense cube (LR::aux_image_cube, built
 * by the reference's own calculate_from_pixelcloud), aux_min / aux_max / aux_area and slide_idx; the two classes' calculate + save_value
 * through their reduce(), with an Fsettings filled as the reference's own 3-D GLCM regression test fills it.  D3_GLCM_feature::offset and
 * ::symmetric_glcm are class statics that nothing in the reference assigns: the driver sets them from settings.glcm_offset / glcm_symmetric.
 *   out[r * 455 ..]   36 intensity codes (Feature3D order) | 30 angled GLCM codes x 13 directions (code-major) | 29 _AVE codes
 * as the classes leave them (NaN / inf are NOT replaced).  assigned[0 .. 29) = 1 where save_value wrote the _AVE code (read off a
 * sentinel), when assigned != NULL.  An ROI without voxels is refused (return 4).
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
#include "features/3d_intensity.h"
#include "features/3d_glcm.h"

#include "nyxhip.h"

using namespace Nyxus;

static const int N_DIR = 13, N_INT = 36, N_ANG = 30, N_AVE = 29, N_COL = N_INT + N_ANG * N_DIR + N_AVE;

extern "C" int volref_batch(const nyxhip_batch3d* b, const nyxhip_settings* s, int n_threads, double* out, int* assigned, double* seconds)
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
        fst[(int)NyxSetting::GLCM_GREYDEPTH].ival = s->glcm_grey_depth;
        fst[(int)NyxSetting::GLCM_OFFSET].ival = s->glcm_offset;
        fst[(int)NyxSetting::GLCM_SPARSEINTENS].bval = true;
        D3_GLCM_feature::offset = s->glcm_offset;
        D3_GLCM_feature::symmetric_glcm = s->glcm_symmetric != 0;
        Dataset ds;
        const bool slide = b->slide_min && b->slide_max;
        if (slide)
            ds.dataset_props.reserve(b->n_roi);
        std::vector<int> L;
        std::unordered_map<int, LR> roiData;
        L.reserve(b->n_roi);
        roiData.reserve(b->n_roi);
        const double SENTINEL = -1234567.25;
        for (uint64_t r = 0; r < b->n_roi; r++) {
            int lab = (int)r + 1;
            L.push_back(lab);
            LR& lr = roiData[lab];
            lr.label = lab;
            uint64_t o = b->px_offset[r], n = b->px_offset[r + 1] - o;
            lr.raw_pixels_3D.reserve(n);
            for (uint64_t i = 0; i < n; i++)
                lr.raw_pixels_3D.push_back(Pixel3((StatsInt)b->x[o + i], (StatsInt)b->y[o + i], (StatsInt)b->z[o + i], (PixIntens)b->inten[o + i]));
            lr.aux_area = (unsigned int)n;
            lr.aux_min = b->min_inten[r];
            lr.aux_max = b->max_inten[r];
            lr.ph_aabb.init_x(0); lr.ph_aabb.update_x((StatsInt)b->bbox_w[r] - 1);
            lr.ph_aabb.init_y(0); lr.ph_aabb.update_y((StatsInt)b->bbox_h[r] - 1);
            lr.ph_aabb.init_z(0); lr.ph_aabb.update_z((StatsInt)b->bbox_d[r] - 1);
            lr.make_nonanisotropic_aabb();
            lr.slide_idx = -1;
            if (slide) {
                SlideProps& sp = ds.dataset_props.emplace_back("", "");
                sp.min_preroi_inten = b->slide_min[r];
                sp.max_preroi_inten = b->slide_max[r];
                lr.slide_idx = (int)r;
            }
            lr.aux_image_cube.calculate_from_pixelcloud(lr.raw_pixels_3D, lr.aabb);
            lr.initialize_fvals();
            for (int k = 0; k < N_AVE; k++)
                lr.fvals[(int)Feature3D::GLCM_ASM_AVE + k][0] = SENTINEL;
        }
        size_t jobSize = L.size(), workPerThread = jobSize / (size_t)n_threads;
        auto a0 = std::chrono::steady_clock::now();
        runParallel(D3_VoxelIntensityFeatures::reduce, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        runParallel(D3_GLCM_feature::reduce, n_threads, workPerThread, jobSize, &L, &roiData, fst, ds);
        auto a1 = std::chrono::steady_clock::now();
        if (seconds)
            seconds[0] = std::chrono::duration<double>(a1 - a0).count();
        if (assigned)
            for (int k = 0; k < N_AVE; k++)
                assigned[k] = 1;
        for (uint64_t r = 0; r < b->n_roi; r++) {
            LR& lr = roiData[(int)r + 1];
            double* o = out + r * N_COL;
            for (int i = 0; i < N_INT; i++)
                o[i] = lr.fvals[(int)Feature3D::COV + i][0];
            for (int c = 0; c < N_ANG; c++) {
                const std::vector<double>& v = lr.fvals[(int)Feature3D::GLCM_ACOR + c];
                if ((int)v.size() != N_DIR)
                    return 5;
                for (int k = 0; k < N_DIR; k++)
                    o[N_INT + c * N_DIR + k] = v[k];
            }
            for (int k = 0; k < N_AVE; k++) {
                o[N_INT + N_ANG * N_DIR + k] = lr.fvals[(int)Feature3D::GLCM_ASM_AVE + k][0];
                if (assigned && o[N_INT + N_ANG * N_DIR + k] == SENTINEL)
                    assigned[k] = 0;
            }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "volref_batch: %s\n", e.what());
        return 2;
    }
    return 0;
}
