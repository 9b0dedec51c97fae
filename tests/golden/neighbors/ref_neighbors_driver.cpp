/*
 * ref_neighbors_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp and tests/golden/circle/ref_circle_driver.cpp) around the
 * reference's own NeighborsFeature.  make_neighbors_golden.py compiles it OUTSIDE the repository against the reference sources where
 * they lie and records what it returns into the fixtures next to this file; nothing compiled from it is kept.
 *
 * The rows [image_offset[k], image_offset[k + 1]) of a host nyxhip_batch are the ROIs of image k, keyed by their roi_label, placed at
 * (origin_x[r], origin_y[r]).  Per image: an LR per ROI with ABSOLUTE pixel coordinates in the batch's cloud order and zeroed fvals;
 * BasicMorphologyFeatures (CENTROID_X / _Y), ContourFeature (LR::multicontour_), then NeighborsFeature::manual_reduce over the image's
 * Roidata with PIXELDISTANCE = pixel_distance:
 *   out[r * 12 ..]  NUM_NEIGHBORS .. ANG_BW_NEIGHBORS_MODE (enum order), the length of the merged multicontour, CENTROID_X, CENTROID_Y
 * seconds[0] = NeighborsFeature::manual_reduce over all images (wall; the class runs on one thread), when seconds != NULL.
 */
#define _USE_MATH_DEFINES
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>
#include <unordered_map>
#include <unordered_set>

#include "roi_cache.h"
#include "dataset.h"
#include "parallel.h"
#include "globals.h"
#include "helpers/helpers.h"
#include "features/basic_morphology.h"
#include "features/contour.h"
#include "features/neighbors.h"

#include "nyxhip.h"

using namespace Nyxus;

extern "C" int neighborsref_batch(const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y, const uint64_t* image_offset,
                                  uint64_t n_images, int pixel_distance, double* out, double* seconds)
{
    if (!b || !out || !image_offset || b->memory != NYXHIP_MEM_HOST || pixel_distance < 1)
        return 1;
    try {
        Fsettings fst;
        fst.resize((int)NyxSetting::__COUNT__);
        fst[(int)NyxSetting::SOFTNAN].rval = 0.0;
        fst[(int)NyxSetting::TINY].rval = 1e-10;
        fst[(int)NyxSetting::SINGLEROI].bval = false;
        fst[(int)NyxSetting::GREYDEPTH].ival = 64;
        fst[(int)NyxSetting::PIXELSIZEUM].rval = 1.0;
        fst[(int)NyxSetting::PIXELDISTANCE].ival = pixel_distance;
        fst[(int)NyxSetting::XYRES].rval = 0.0;
        fst[(int)NyxSetting::USEGPU].bval = false;
        fst[(int)NyxSetting::VERBOSLVL].ival = 0;
        fst[(int)NyxSetting::IBSI].bval = false;
        Dataset ds;
        double sec = 0.0;
        static const Feature2D codes[9] = {Feature2D::NUM_NEIGHBORS, Feature2D::PERCENT_TOUCHING, Feature2D::CLOSEST_NEIGHBOR1_DIST,
                                           Feature2D::CLOSEST_NEIGHBOR1_ANG, Feature2D::CLOSEST_NEIGHBOR2_DIST, Feature2D::CLOSEST_NEIGHBOR2_ANG,
                                           Feature2D::ANG_BW_NEIGHBORS_MEAN, Feature2D::ANG_BW_NEIGHBORS_STDDEV, Feature2D::ANG_BW_NEIGHBORS_MODE};
        for (uint64_t k = 0; k < n_images; k++) {
            std::vector<int> L;
            Roidata roiData;
            std::unordered_set<int> uniq;
            for (uint64_t r = image_offset[k]; r < image_offset[k + 1]; r++) {
                const int lab = (int)b->roi_label[r];
                if (!uniq.insert(lab).second)
                    return 3;                                    // a label twice in one image
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
            if (L.empty())
                continue;
            runParallel(ContourFeature::reduce, 1, L.size(), L.size(), &L, &roiData, fst, ds);
            auto a0 = std::chrono::steady_clock::now();
            NeighborsFeature::manual_reduce(roiData, fst, uniq);
            sec += std::chrono::duration<double>(std::chrono::steady_clock::now() - a0).count();
            for (uint64_t r = image_offset[k]; r < image_offset[k + 1]; r++) {
                LR& lr = roiData[(int)b->roi_label[r]];
                double* o = out + r * 12;
                for (int i = 0; i < 9; i++)
                    o[i] = lr.fvals[(int)codes[i]][0];
                std::vector<Pixel2> K;
                lr.merge_multicontour(K);
                o[9] = (double)K.size();
                o[10] = lr.fvals[(int)Feature2D::CENTROID_X][0];
                o[11] = lr.fvals[(int)Feature2D::CENTROID_Y][0];
            }
        }
        if (seconds) seconds[0] = sec;
    } catch (const std::exception& e) {
        fprintf(stderr, "neighborsref_batch: %s\n", e.what());
        return 2;
    }
    return 0;
}
