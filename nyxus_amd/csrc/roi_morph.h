// roi_morph.h -- host/device interface of the 2-D morphology unit (roi_morph.hip): BasicMorphologyFeatures, ContourFeature,
// ConvexHullFeature and ExtremaFeature of the reference's shape block.  A header of its own, like roi_caliper.h and roi_circle.h.
#pragma once
#include "roi_kernel.h"

namespace nyxhip {

constexpr int kMorphBasicCols = 15;        // AREA_PIXELS_COUNT .. ASPECT_RATIO (featureset.h:46-60 of the reference)
constexpr int kMorphContourCols = 7;       // PERIMETER .. EDGE_INTEGRATED_INTENSITY (:71-77)
constexpr int kMorphHullCols = 3;          // CIRCULARITY, CONVEX_HULL_AREA, SOLIDITY (:78-82)
constexpr int kMorphExtremaCols = 16;      // EXTREMA_P1_X, EXTREMA_P1_Y .. EXTREMA_P8_X, EXTREMA_P8_Y (:136-143)
constexpr int kMorphCols = kMorphBasicCols + kMorphContourCols + kMorphHullCols + kMorphExtremaCols;
constexpr uint32_t kMorphColsLds = 1024;   // upper bound of MorphArgs::cols_cap: box columns whose tables the kernel keeps in LDS (kCaliperColsLds)
constexpr uint32_t kMorphBytesPerCol = 24; // min_y | max_y (8 B), lower chain (8 B), upper chain / hull (8 B)
constexpr uint32_t kMorphPlaneLds = 8192;  // upper bound of MorphArgs::plane_cap: box cells of the u32 intensity plane the kernel keeps in LDS

__host__ __device__ inline int morph_n_columns(uint32_t m)
{
    return ((m & NYXHIP_MORPH_BASIC) ? kMorphBasicCols : 0) + ((m & NYXHIP_MORPH_CONTOUR) ? kMorphContourCols : 0) +
           ((m & NYXHIP_MORPH_HULL) ? kMorphHullCols : 0) + ((m & NYXHIP_MORPH_EXTREMA) ? kMorphExtremaCols : 0);
}

struct MorphArgs {
    uint64_t n_roi;
    const uint64_t* px_offset;
    const uint16_t* x;
    const uint16_t* y;
    const uint32_t* inten;
    const uint32_t* bbox_w;
    const uint32_t* bbox_h;
    const uint32_t* origin_x;  // [n_roi] aabb.xmin / aabb.ymin of the ROI in its image, or NULL: (0, 0)
    const uint32_t* origin_y;
    const uint32_t* ws_contour;   // the contour chain's workspace (MomArgs::ws_contour / n_contour); NULL when neither CONTOUR nor HULL is asked for
    const uint32_t* n_contour;
    double* out;
    uint64_t ld;
    int* status;
    uint32_t morph;            // subset of NYXHIP_MORPH_ALL
    int32_t col_basic, col_contour, col_hull, col_extrema;   // first column of each class inside the output row
    const uint32_t* roi_index; // NULL: workgroup b serves ROI b; else ROI roi_index[b] (the boxes beyond the LDS carve)
    uint32_t cols_cap;         // box columns of tables behind the kernel's dynamic LDS
    uint32_t plane_cap;        // box cells of the intensity plane behind them
    uint32_t defer_big;        // 1: skip the ROIs beyond either cap (a launch over their list, with ws, follows)
    unsigned char* ws;         // list launches: per workgroup kMorphBytesPerCol * ws_cols bytes of tables, then 4 * ws_cells bytes of plane
    uint32_t ws_cols;
    uint64_t ws_cells, ws_stride;
};

int launch_roi_morph(const MorphArgs& a, void* stream, uint32_t grid);
// predicate of the deferred list (deferred_list.h): ROIs whose box is wider than `cols` columns or holds more than `cells` cells;
// header word 1 = the widest listed box, words 2 and 3 = the largest listed height and width (their product bounds the cells)
struct MorphBig { const uint32_t *bw, *bh; uint32_t cols, cells; __device__ bool operator()(uint64_t i, uint32_t* hdr) const; };

} // namespace nyxhip
