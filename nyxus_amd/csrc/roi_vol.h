// roi_vol.h -- host/device interface of the volume unit (roi_vol.hip): the voxel-intensity block and the 3-D GLCM block of the
// reference's Feature3D enum (D3_VoxelIntensityFeatures, D3_GLCM_feature).  A header of its own, like roi_imq.h.  The classes claim no bit
// of the 2-D family mask: their table belongs to nyxhip_featurize_volumes (nyxhip_vol.hip).
#pragma once
#include <stdint.h>

namespace nyxhip {

constexpr int kVolIntensityCols = 36;      // Feature3D COV .. UNIFORMITY_PIU (featureset.h:646-676)
constexpr int kVolDirs = 13;               // shifts[] of 3d_glcm.cpp:16-31
constexpr int kVolGlcmAngled = 30;         // Feature3D GLCM_ACOR .. GLCM_VARIANCE (:739-768)
constexpr int kVolGlcmAve = 29;            // Feature3D GLCM_ASM_AVE .. GLCM_SUMVARIANCE_AVE (:769-797)
constexpr int kVolGlcmCols = kVolGlcmAngled * kVolDirs + kVolGlcmAve;
// THE LDS BUDGET of vol_glcm_kernel, at the level cap: the co-occurrence matrix 128 x 128 x 4 B = 64 KiB, the staged binned box
// kVolLdsCells x 1 B = 32 KiB, the closing routine's marginals 5 x 128 x 8 B = 5 KiB, level values 1 KiB, level map 256 B, results
// 256 B: 103 KiB of the 160 KiB a gfx950 workgroup may claim.
constexpr uint32_t kVolLevelCap = 128;
// THE SWITCH-OVER, by the cells w * h * d of the ROI's own box (never by what else shares the launch):
//   cells <= kVolLdsCells   the binned box is staged in LDS and the pair sweep reads it there
//   beyond                  the pair sweep reads the binned box in the global workspace
constexpr uint32_t kVolLdsCells = 32768;
constexpr uint32_t kVolMaxCells = 1u << 24;
constexpr uint32_t kVolMaxSide = 65534;

struct VolArgs {
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
    const double* slide_min;               // or NULL
    const double* slide_max;
    int grey_info;                         // GLCM binning: 0 IBSI, > 0 matlab levels, < 0 radiomics bins (3d_glcm.cpp:51-53)
    int offset;                            // D3_GLCM_feature::offset
    int symmetric;                         // D3_GLCM_feature::symmetric_glcm
    uint32_t n_hist;                       // |grey_depth|: bins of the intensity histogram
    double soft_nan;
    double* out;                           // [n_roi of the BATCH x ld]
    uint64_t ld;
    int col_intensity, col_glcm;           // first column of each block in a row (-1: not requested)
    int* status;
    unsigned char* boxes;                  // binned boxes of the chunk, box_stride bytes each (level indices, one byte per cell)
    uint64_t box_stride;
    uint32_t* keys;                        // two sort buffers of key_stride words per ROI of the chunk, back to back
    uint64_t key_stride;
    uint32_t max_cells, max_px;            // what the strides were sized for: an ROI beyond them is NYXHIP_ERR_ROI_TOO_LARGE
    uint32_t stage_cells;                  // cells of the LDS staging area of this launch (min(max_cells, kVolLdsCells), 16-aligned)
    uint32_t ng_bound;                     // matrix order the LDS of this launch holds (<= kVolLevelCap)
};

// Every function enqueues on `stream` and returns a hipError_t as int.
int launch_vol_bin(const VolArgs& a, void* stream);         // binned boxes of the chunk (the caller has filled them with the background level)
int launch_vol_glcm(const VolArgs& a, void* stream);        // one workgroup per (ROI, direction), then the _AVE columns
int launch_vol_intensity(const VolArgs& a, void* stream);   // one workgroup per ROI
int vol_background_level(int grey_info);                    // level of a cell outside the cloud (matlab binning maps 0 to 1)

} // namespace nyxhip
