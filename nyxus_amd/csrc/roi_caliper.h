// roi_caliper.h -- host/device interface of the caliper kernel (roi_caliper.hip): Feret, Martin and Nassenstein diameters.
// A header of its own, like roi_radial.h and roi_outline.h.
#pragma once
#include "roi_kernel.h"

namespace nyxhip {

constexpr int kFeretCols = 8;              // MIN_FERET_ANGLE, MAX_FERET_ANGLE, STAT_FERET_DIAM_{MIN,MAX,MEAN,MEDIAN,STDDEV,MODE}
constexpr int kMartinCols = 6;             // STAT_MARTIN_DIAM_{MIN,MAX,MEAN,MEDIAN,STDDEV,MODE}
constexpr int kNassensteinCols = 6;        // STAT_NASSENSTEIN_DIAM_{...}
constexpr int kCaliperAngles = 19;         // theta = 0, 10, ..., 180 (Feret: all 19; Martin and Nassenstein: theta < 180, the first 18)
constexpr int kMartinLevels = 100;         // NGRID of caliper_martin.cpp:101
constexpr uint32_t kCaliperColsLds = 1024; // upper bound of CalArgs::cols_cap: box columns whose tables the kernel keeps in LDS
constexpr uint32_t kCaliperBytesPerCol = 24;   // min_y | max_y | lower chain (16 B, the rotated vertices afterwards), upper chain / hull (8 B)

struct CalArgs {
    uint64_t n_roi;
    const uint64_t* px_offset;
    const uint16_t* x;
    const uint16_t* y;
    const uint32_t* bbox_w;
    const uint32_t* origin_x;  // [n_roi] aabb.xmin / aabb.ymin of the ROI in its image, or NULL: (0, 0)
    const uint32_t* origin_y;
    double* out;
    uint64_t ld;
    int* status;
    uint32_t fams;             // subset of NYXHIP_FAM_FERET | NYXHIP_FAM_MARTIN | NYXHIP_FAM_NASSENSTEIN
    int32_t col_feret, col_martin, col_nassenstein;   // first column of each class inside the output row
    double soft_nan;
    const uint32_t* roi_index; // NULL: workgroup b serves ROI b; else ROI roi_index[b] (the wide boxes of a batch)
    uint32_t cols_cap;         // box columns of tables behind the kernel's dynamic LDS
    uint32_t defer_wide;       // 1: skip the ROIs whose boxes are wider than cols_cap (a launch over their list, with ws, follows)
    unsigned char* ws;         // list launches: kCaliperBytesPerCol * ws_cols bytes of global scratch per workgroup
    uint32_t ws_cols;
    // sin / cos of the 19 angles, filled on the host with the reference's expression (rotation.cpp:56-58) through the host's libm
    double sn[kCaliperAngles], cs[kCaliperAngles];
};

int launch_roi_caliper(const CalArgs& a, void* stream, uint32_t grid);
// predicate of the deferred list (deferred_list.h): ROIs whose boxes are wider than `cap` columns
struct CaliperWide { const uint32_t* bw; uint32_t cap; __device__ bool operator()(uint64_t i, uint32_t* hdr) const; };

} // namespace nyxhip
