// roi_voltex.h -- host/device interface of the volume texture unit (roi_voltex.hip): the GLDM, NGLDM and NGTDM blocks of the reference's
// Feature3D enum (D3_GLDM_feature, D3_NGLDM_feature, D3_NGTDM_feature).  The table belongs to nyxhip_featurize_volumes_tex
// (nyxhip_voltex.hip); the batch type, the binned-box workspace and vol_bin_kernel are those of roi_vol.h.
#pragma once
#include <stdint.h>

namespace nyxhip {

constexpr int kVtGldmCols = 14;            // Feature3D GLDM_SDE .. GLDM_LDHGLE
constexpr int kVtNgldmCols = 19;           // Feature3D NGLDM_LDE .. NGLDM_DCENE
constexpr int kVtNgtdmCols = 5;            // Feature3D NGTDM_COARSENESS .. NGTDM_STRENGTH
constexpr uint32_t kVtLevelCap = 128;      // NYXHIP_VOLTEX_MAX_LEVELS
constexpr uint32_t kVtRows = kVtLevelCap + 1;   // a table row per level 0 .. cap (NGTDM's +1 is applied to the level VALUES in the closing)
constexpr uint32_t kVtGldmDeps = 27;       // dependence counts 1 .. 27 (26 shifts and the voxel itself, 3d_gldm.cpp:133)
constexpr uint32_t kVtNgldmDeps = 25;      // matches 0 .. 24 (3d_ngldm.cpp:144-156)
constexpr int kVtMaxRadius = 3;            // NYXHIP_VOLTEX_MAX_RADIUS
constexpr uint32_t kVtMaxClasses = 64;     // (radius + 1)^3 neighbourhood classes at the radius cap
// THE CELL RANGE of one workgroup of a sweep, in cells of the ROI's own box in raster order: workgroup k of an ROI owns the cells
// [k * kVtCellsPerWg, (k + 1) * kVtCellsPerWg).  Sized by the ROI alone, never by what shares the launch.
constexpr uint32_t kVtCellsPerWg = 32768;

// A per-ROI table, in 32-bit words: [0, 8) the presence map of the levels of the binned box (bit l = level l occurs in a cell), then
//   GLDM    [level][dependence - 1]  counts
//   NGLDM   [level][matches]         counts
//   NGTDM   [level] counts (kVtRows words, padded to kVtNgtdmSums), then 64-bit sums [level][class] of |nd * i - sum of the neighbours|
constexpr uint32_t kVtTabHead = 8;
constexpr uint32_t kVtGldmWords = kVtTabHead + kVtRows * kVtGldmDeps;
constexpr uint32_t kVtNgldmWords = kVtTabHead + kVtRows * kVtNgldmDeps;
constexpr uint32_t kVtNgtdmSums = kVtTabHead + kVtRows + 1;   // even: the 64-bit sums are 8-byte aligned
__host__ __device__ inline uint32_t vt_classes(int radius) { return (uint32_t)((radius + 1) * (radius + 1) * (radius + 1)); }
__host__ __device__ inline uint32_t vt_ngtdm_words(int radius) { return kVtNgtdmSums + 2u * kVtRows * vt_classes(radius); }
// THE LDS BUDGET of a sweep workgroup is its table: GLDM 13.7 KiB, NGLDM 12.7 KiB, NGTDM 0.5 KiB + 1 KiB per class (8.6 / 27.8 / 65.1 KiB
// at radius 1 / 2 / 3).  The closing keeps one table and 3 x kVtRows doubles: under 17 KiB.

enum { VT_GLDM = 0, VT_NGLDM = 1, VT_NGTDM = 2 };

struct VoltexArgs {
    uint64_t roi0, n_roi;                  // the ROIs [roi0, roi0 + n_roi) of the batch: one chunk
    const uint64_t* px_offset;
    const uint16_t* x;
    const uint16_t* y;
    const uint16_t* z;
    const uint32_t* inten;
    const uint32_t* bbox_w;
    const uint32_t* bbox_h;
    const uint32_t* bbox_d;
    const uint32_t* vmin;                  // LR::aux_min
    const uint32_t* vmax;                  // LR::aux_max
    int ibsi;
    int g_gldm, g_ngtdm;                   // greyInfo of the two classes: 0 none, > 0 matlab levels, < 0 radiomics bins
    uint32_t ngldm_levels;                 // grey_depth as to_grayscale reads it (unsigned)
    int radius;                            // NGTDM: Chebyshev radius of the cube
    double soft_nan;
    double* out;                           // [n_roi of the BATCH x ld]
    uint64_t ld;
    int col_gldm, col_ngldm, col_ngtdm;    // first column of each block in a row (-1: not requested)
    int* status;
    unsigned char* box[3];                 // binned boxes of the chunk per class (VT_*), box_stride bytes per ROI; GLDM and NGTDM may share
    uint64_t box_stride;
    uint32_t* tab[3];                      // per-ROI tables of the chunk per class, tab_stride[c] words per ROI (zeroed by the caller)
    uint64_t tab_stride[3];
    uint32_t max_cells;                    // what box_stride was sized for
};

// Every function enqueues on `stream` and returns a hipError_t as int.
int launch_voltex_bin_ngldm(const VoltexArgs& a, uint32_t max_px, void* stream);   // box[VT_NGLDM] (the caller has filled it with 0)
int launch_voltex_sweep(const VoltexArgs& a, int cls, void* stream);               // tab[cls] from box[cls]
int launch_voltex_ngtdm_r0(const VoltexArgs& a, void* stream);                     // the NGTDM block at radius 0, from the cloud
int launch_voltex_close(const VoltexArgs& a, void* stream);                        // the columns from the tables

} // namespace nyxhip
