// roi_erosion.h -- host/device interface of the erosion / ellipse unit (roi_erosion.hip): EROSIONS_2_VANISH[_COMPLEMENT] and the six
// columns of EllipseFittingFeature.  A header of its own, like roi_radial.h, roi_outline.h, roi_caliper.h and roi_chords.h.
#pragma once
#include "roi_kernel.h"

namespace nyxhip {

constexpr int kEllipseCols = 6;            // MAJOR_AXIS_LENGTH, MINOR_AXIS_LENGTH, ELONGATION, ECCENTRICITY, ORIENTATION, ROUNDNESS
constexpr int kErosionCols = 2;            // EROSIONS_2_VANISH, EROSIONS_2_VANISH_COMPLEMENT
constexpr int kErosionMaxPasses = 1000;    // SANITY_MAX_NUM_EROSIONS (erosion.h)
// THE SWITCH-OVER: an ROI whose TWO bit planes (rows of w / 32 + 1 words, h rows, twice) exceed this many 32-bit words (32 KiB of
// LDS) is eroded on global planes (classifier + list launch).
constexpr uint32_t kErosionLdsWords = 8192;
// Ellipse: an ROI of at most this many pixels is summed by one wave (four ROIs per workgroup), a larger one by a workgroup.
constexpr uint32_t kEllipseWavePx = 2048;

// words of ONE bit plane of a w x h box
__host__ __device__ inline uint64_t erosion_plane_words(uint32_t w, uint32_t h)
{
    return (uint64_t)(w / 32u + 1u) * h;
}

struct EroArgs {
    uint64_t n_roi;
    const uint64_t* px_offset;
    const uint16_t* x;
    const uint16_t* y;
    const uint32_t* bbox_w;
    const uint32_t* bbox_h;
    const uint32_t* min_inten;
    const uint32_t* max_inten;
    double* out;
    uint64_t ld;
    int* status;
    int32_t col_ellipse;       // first of the 6 ellipse columns inside the output row
    int32_t col_erosion;       // first of the 2 erosion columns
    uint32_t lds_words;        // words of the two planes behind the erosion kernel's dynamic LDS (<= kErosionLdsWords)
    uint32_t defer_large;      // 1: skip the ROIs whose two planes exceed lds_words (a launch over their list, with ws, follows)
    const uint32_t* roi_index; // NULL: workgroup b serves ROI b; else ROI roi_index[b], on global planes
    uint32_t* ws;              // list launches: ws_stride words of global scratch per workgroup (two planes)
    uint64_t ws_stride;
};

int launch_roi_erosion(const EroArgs& a, void* stream, uint32_t grid);
// predicate of the deferred list (deferred_list.h): ROIs whose two planes exceed `cap` words; hdr[1] = largest plane among them
// (words of ONE plane, saturated)
struct ErosionListed { const uint32_t *bw, *bh; uint32_t cap; __device__ bool operator()(uint64_t i, uint32_t* hdr) const; };
// the ellipse columns of every ROI: a wave per ROI of <= kEllipseWavePx pixels, and, when `with_large`, a workgroup per larger ROI
int launch_roi_ellipse(const EroArgs& a, void* stream, bool with_large);

} // namespace nyxhip
