// roi_hexpoly.h -- host/device interface of the closing kernel of HexagonalityPolygonalityFeature (roi_hexpoly.hip): POLYGONALITY_AVE,
// HEXAGONALITY_AVE, HEXAGONALITY_STDDEV.  A header of its own, like roi_neighbors.h and roi_morph.h.  The class is a formula over six
// per-ROI numbers that other kernels produce; hexpoly_device (nyxhip_hexpoly.hip) lets them write into one scratch table whose columns
// are named here.
#pragma once
#include "roi_kernel.h"
#include "roi_neighbors.h"
#include "roi_morph.h"
#include "roi_caliper.h"

namespace nyxhip {

constexpr int kHexpolyCols = 3;            // POLYGONALITY_AVE, HEXAGONALITY_AVE, HEXAGONALITY_STDDEV (featureset.h:146-148 of the reference)
constexpr int kHexpolyTanCap = 128;        // tan(M_PI / k), k = 3 .. kHexpolyTanCap, comes from the host's libm (HexArgs::tan_tab); beyond: the device's tan
// the scratch table [n_roi x kHexpolyInLd]: the neighbor columns | the CONTOUR and HULL columns of the morphology kernel | the Feret columns
constexpr int kHexpolyInNeighbors = 0;
constexpr int kHexpolyInMorph = kHexpolyInNeighbors + kNeighborCols;
constexpr int kHexpolyInFeret = kHexpolyInMorph + kMorphContourCols + kMorphHullCols;
constexpr int kHexpolyInLd = kHexpolyInFeret + kFeretCols;
constexpr int kHexpolyInNumNeighbors = kHexpolyInNeighbors;                   // NUM_NEIGHBORS
constexpr int kHexpolyInPerimeter = kHexpolyInMorph;                          // PERIMETER
constexpr int kHexpolyInHullArea = kHexpolyInMorph + kMorphContourCols + 1;   // CONVEX_HULL_AREA (behind CIRCULARITY)
constexpr int kHexpolyInFeretMin = kHexpolyInFeret + 2;                       // STAT_FERET_DIAM_MIN (behind the two angles)
constexpr int kHexpolyInFeretMax = kHexpolyInFeret + 3;                       // STAT_FERET_DIAM_MAX

struct HexArgs {
    uint64_t n_roi;
    const uint64_t* px_offset;     // the pixel count is the reference's `area` (aux_area)
    const uint32_t* n_contour;     // the contour chain's lengths (MomArgs::n_contour): 0 is the first gate
    const double* in;              // [n_roi x kHexpolyInLd], the columns above
    const double* tan_tab;         // [kHexpolyTanCap + 1], entry k = tan(M_PI / k) of the host's libm (entries 0 .. 2 are never read)
    double* out;                   // [n_roi x ld], kHexpolyCols columns
    uint64_t ld;
};

int launch_roi_hexpoly(const HexArgs& a, void* stream);

} // namespace nyxhip
