// roi_outline.h -- host/device interface of the outline kernel (roi_outline.hip): fractal dimensions, Euler number, ROI radius.
// A header of its own, like roi_radial.h: roi_kernel.h is one of the sources the measured HBM traffic of the metric kernels is
// keyed on, and these families touch none of them.
#pragma once
#include "roi_kernel.h"

namespace nyxhip {

constexpr int kFractalCols = 2;           // FRACT_DIM_BOXCOUNT, FRACT_DIM_PERIMETER
constexpr int kEulerCols = 1;             // EULER_NUMBER
constexpr int kRoiRadiusCols = 3;         // ROI_RADIUS_MEAN, ROI_RADIUS_MAX, ROI_RADIUS_MEDIAN
constexpr uint32_t kOutlineBitsLds = 2048;   // upper bound of OutArgs::bits_cap: 32-bit words of bit planes the kernel keeps in LDS

// smallest power of two >= a (helpers.h:241-248)
__host__ __device__ inline uint32_t outline_ceil_pow2(uint32_t a)
{
    if (a <= 1) return 1;
    uint32_t x = a - 1;
    x |= x >> 1; x |= x >> 2; x |= x >> 4; x |= x >> 8; x |= x >> 16;
    return x + 1;
}

// Words of the ROI's bit planes: the mask of the w x h box, one bit per cell, rows of w / 32 + 1 words (the bit behind the last
// column exists and is 0: the quad scan of the Euler number reads it), and, with `pyramid`, the box occupancy of every box size
// 2, 4, ..., ceil_pow2(max(w, h)) behind it (level k: every dimension of level k - 1 halved, rounded up).
__host__ __device__ inline uint64_t outline_bit_words(uint32_t w, uint32_t h, bool pyramid)
{
    uint64_t wd = w / 32u + 1u, rows = h, total = wd * rows;
    if (pyramid)
        for (uint32_t s = outline_ceil_pow2(w > h ? w : h); s > 1; s >>= 1) {
            wd = (wd + 1) / 2; rows = (rows + 1) / 2;
            total += wd * rows;
        }
    return total;
}

struct OutArgs {
    MomArgs m;                // batch, contour workspace, LDS carve (pixels | contour | step table) and launch filter of the moments launches
    uint32_t fams;            // subset of NYXHIP_FAM_FRACTAL | NYXHIP_FAM_EULER | NYXHIP_FAM_ROI_RADIUS
    int32_t col_fractal, col_euler, col_radius;   // first column of each family inside the output row
    uint32_t has_contour;     // 0: an Euler-only call -- no contour was computed, m.ws_contour / m.n_contour are not read
    uint32_t bits_cap;        // words of bit planes behind the step table in LDS
    uint32_t defer_bits;      // 1: skip the ROIs whose bit planes exceed bits_cap (a launch over their list, with bits_ws, follows)
    uint32_t* bits_ws;        // list launches: bits_stride words of global scratch per workgroup
    uint64_t bits_stride;
};

int launch_roi_outline(const OutArgs& a, void* stream, uint32_t grid);
// predicate of the deferred list (deferred_list.h): ROIs whose bit planes exceed `cap` words
struct OutlineBitsBig { const uint32_t *bw, *bh; uint32_t pyramid, cap; __device__ bool operator()(uint64_t i, uint32_t* hdr) const; };

} // namespace nyxhip
