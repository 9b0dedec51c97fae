/*
 * ref_hexpoly_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A thin driver (own code, in the manner of oracle/ref_driver.cpp and tests/golden/morph/ref_morph_driver.cpp) around the
 * reference's own HexagonalityPolygonalityFeature.  make_hexpoly_golden.py compiles it OUTSIDE the repository against the reference
 * sources where they lie and records what it returns into the fixtures next to this file; nothing compiled from it is kept.
 *
 * The class is a closing formula over values other classes left in the ROI's cache, so the driver fills exactly those: per row r of
 * `in` [n x 7] = N_PIXELS, N_CONTOUR, NUM_NEIGHBORS, PERIMETER, CONVEX_HULL_AREA, STAT_FERET_DIAM_MIN, STAT_FERET_DIAM_MAX an LR
 * with aux_area, the five fvals, and a dummy multicontour_ of N_CONTOUR points where N_CONTOUR > 0 (the class only asks whether it
 * is empty).  Then the class's batch reducer, gates included:
 *   out[r * 3 ..]   POLYGONALITY_AVE, HEXAGONALITY_AVE, HEXAGONALITY_STDDEV, RAW (NaN and infinities stay)
 */
#define _USE_MATH_DEFINES
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include <unordered_map>

#include "roi_cache.h"
#include "dataset.h"
#include "features/hexagonality_polygonality.h"

using namespace Nyxus;

extern "C" int hexpolyref_rows(const double* in, uint64_t n, double* out)
{
    if (!in || !out)
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
        L.reserve(n);
        roiData.reserve(n);
        for (uint64_t r = 0; r < n; r++) {
            const double* v = in + r * 7;
            int lab = (int)r + 1;
            L.push_back(lab);
            LR& lr = roiData[lab];
            lr.label = lab;
            lr.aux_area = (unsigned int)v[0];
            lr.aux_min = 1;
            lr.aux_max = 2;
            lr.slide_idx = -1;
            lr.initialize_fvals();
            const uint64_t nk = (uint64_t)v[1];
            if (nk)
                lr.multicontour_.push_back(std::vector<Pixel2>(nk, Pixel2(0, 0, 0)));
            lr.fvals[(int)Feature2D::NUM_NEIGHBORS][0] = v[2];
            lr.fvals[(int)Feature2D::PERIMETER][0] = v[3];
            lr.fvals[(int)Feature2D::CONVEX_HULL_AREA][0] = v[4];
            lr.fvals[(int)Feature2D::STAT_FERET_DIAM_MIN][0] = v[5];
            lr.fvals[(int)Feature2D::STAT_FERET_DIAM_MAX][0] = v[6];
        }
        HexagonalityPolygonalityFeature::parallel_process_1_batch(0, L.size(), &L, &roiData, fst, ds);
        for (uint64_t r = 0; r < n; r++) {
            LR& lr = roiData[(int)r + 1];
            out[r * 3 + 0] = lr.fvals[(int)Feature2D::POLYGONALITY_AVE][0];
            out[r * 3 + 1] = lr.fvals[(int)Feature2D::HEXAGONALITY_AVE][0];
            out[r * 3 + 2] = lr.fvals[(int)Feature2D::HEXAGONALITY_STDDEV][0];
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "hexpolyref_rows: %s\n", e.what());
        return 2;
    }
    return 0;
}
