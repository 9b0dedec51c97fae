// roi_volzone.h -- host/device interface of the volume zone unit (roi_volzone.hip): the GLRLM and GLSZM blocks of the reference's
// Feature3D enum (D3_GLRLM_feature, D3_GLSZM_feature).  The table belongs to nyxhip_featurize_volumes_zones (nyxhip_volzone.hip); the
// batch type, the binned-box workspace and vol_bin_kernel are those of roi_vol.h.
#pragma once
#include <stdint.h>

namespace nyxhip {

constexpr int kVzDirs = 13;                // shifts13[] of 3d_glrlm.cpp:17-32
constexpr int kVzGlrlmCodes = 16;          // Feature3D GLRLM_SRE .. GLRLM_LRHGLE, then as many _AVE codes
constexpr int kVzGlrlmCols = kVzGlrlmCodes * kVzDirs + kVzGlrlmCodes;
constexpr int kVzGlszmCols = 16;           // Feature3D GLSZM_SAE .. GLSZM_LAHGLE
constexpr uint32_t kVzLevelCap = 128;      // NYXHIP_VOLZONE_MAX_LEVELS
// THE CELL RANGE of one workgroup of a sweep, in cells of the ROI's own box in raster order: workgroup k of an ROI owns the cells
// [k * kVzCellsPerWg, (k + 1) * kVzCellsPerWg).  Sized by the ROI alone, never by what shares the launch.
constexpr uint32_t kVzCellsPerWg = 4096;
// Runs up to this length are counted in LDS ([level][length - 1], merged with integer atomics); longer ones go to the global table.
constexpr uint32_t kVzShortRuns = 8;
// Zones up to this size are counted in a dense per-ROI table [level][size - 1]; larger ones become keys of a list that is sorted.
constexpr uint32_t kVzDenseSizes = 32;
constexpr uint32_t kVzNoLabel = 0xFFFFFFFFu;   // label of a background cell

enum { VZ_GLRLM = 0, VZ_GLSZM = 1 };

// Per-ROI words of the GLRLM table: [0, 16) the longest run per direction, then per direction k at rl_dir_off[k] the counts
// [level][length - 1] with the ROI's OWN pitch L_k = the smallest box side among the direction's non-zero components.
constexpr uint32_t kVzRlHead = 16;
// Per-ROI words of the GLSZM table: [0] the number of list keys (arrival counter), [1] which of the two key buffers holds the sorted
// list, then the dense counts [level][size - 1] (pitch kVzDenseSizes).
constexpr uint32_t kVzSzHead = 8;

struct VolzoneArgs {
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
    int g[2];                              // greyInfo of the two classes (VZ_*): 0 none, > 0 matlab levels, < 0 radiomics bins
    uint32_t rows[2];                      // table rows of the call per class: the level bound + 1 (row = level)
    double soft_nan;
    double* out;                           // [n_roi of the BATCH x ld]
    uint64_t ld;
    int col[2];                            // first column of each block in a row (-1: not requested)
    int* status;
    unsigned char* box[2];                 // binned boxes of the chunk per class, box_stride bytes per ROI; may be shared
    uint64_t box_stride;
    uint32_t max_cells;                    // what the strides were sized for
    uint32_t side_max[3];                  // largest w, h, d of the batch: what rl_dir_off was sized for
    uint32_t* rl_tab;                      // GLRLM tables of the chunk, rl_stride words per ROI (zeroed by the caller)
    uint64_t rl_stride;
    uint64_t rl_dir_off[kVzDirs];
    uint32_t* sz_tab;                      // GLSZM tables of the chunk, sz_stride words per ROI (zeroed by the caller)
    uint64_t sz_stride;
    uint32_t* sz_label;                    // a label per cell, cell_stride words per ROI
    uint32_t* sz_count;                    // cells per root, cell_stride words per ROI
    uint64_t cell_stride;
    uint32_t* sz_keys;                     // two key buffers of key_stride words per ROI, back to back
    uint64_t key_stride;
};

__host__ __device__ inline uint32_t vz_min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
// the longest possible run of direction (dz, dy, dx) in a w x h x d box
__host__ __device__ inline uint32_t vz_dir_len(int dz, int dy, int dx, uint32_t w, uint32_t h, uint32_t d)
{
    uint32_t L = 0xFFFFFFFFu;
    if (dz) L = vz_min_u32(L, d);
    if (dy) L = vz_min_u32(L, h);
    if (dx) L = vz_min_u32(L, w);
    return L;
}
extern const int kVzShifts[kVzDirs][3];    // (dz, dy, dx)

// Every function enqueues on `stream` and returns a hipError_t as int.
int launch_volzone_runs(const VolzoneArgs& a, void* stream);        // rl_tab from box[VZ_GLRLM], then the 224 GLRLM columns
int launch_volzone_zones(const VolzoneArgs& a, void* stream);       // labels, sizes, sz_tab and the sorted list from box[VZ_GLSZM], then the 16 columns
// the launches of the GLSZM chain one by one: 0 init, 1 merge, 2 count, 3 emit, 4 sort, 5 close
constexpr int kVzZoneSteps = 6;
int launch_volzone_zone_step(const VolzoneArgs& a, int step, void* stream);

} // namespace nyxhip
