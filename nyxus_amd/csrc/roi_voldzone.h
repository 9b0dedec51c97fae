// roi_voldzone.h -- host/device interface of the volume distance-zone unit (roi_voldzone.hip): the GLDZM block of the reference's
// Feature3D enum (D3_GLDZM_feature).  The table belongs to nyxhip_featurize_volumes_dzones (nyxhip_voldzone.hip); the batch type, the
// binned-box workspace and vol_bin_kernel are those of roi_vol.h, the cell range of a workgroup that of roi_volzone.h.
#pragma once
#include <stdint.h>
#include "roi_volzone.h"

namespace nyxhip {

constexpr int kVdzCols = 18;               // Feature3D GLDZM_SDE .. GLDZM_ZDE (GLE is computed and not saved: 3d_gldzm.cpp:550-570)
// Zones whose metric is up to this are counted in LDS ([level][metric - 1], merged with integer atomics); larger metrics go to the
// global table directly.
constexpr uint32_t kVdzShortDist = 8;
// Per-ROI words of the table: [0] the largest zone metric Nd, then the counts [level][metric - 1] with the ROI's OWN pitch
// vdz_pitch(w, h).
constexpr uint32_t kVdzHead = 8;
// Cells of one wave's job in the x sweeps of the distance map: whole rows, about this many cells.
constexpr uint32_t kVdzRowCells = 1024;

// THE BOUND OF THE METRIC.  Along x a cell's distance is at most min(x + 1, w - x) <= (w + 1) / 2, likewise along y, and a zone's metric
// is the minimum over its cells: no metric exceeds (min(w, h) + 1) / 2 <= min(w, h) / 2 + 2, the pitch of the ROI's table.  With sides
// up to kVolMaxSide = 65534 that is at most 32769: a distance is stored in 16 bits.
__host__ __device__ inline uint32_t vdz_pitch(uint32_t w, uint32_t h) { return (w < h ? w : h) / 2u + 2u; }
// rows of the box one wave sweeps along x
__host__ __device__ inline uint32_t vdz_rows_per_wave(uint32_t w) { return w >= kVdzRowCells ? 1u : kVdzRowCells / w; }

struct VoldzoneArgs {
    uint64_t roi0, n_roi;                  // the ROIs [roi0, roi0 + n_roi) of the batch: one chunk
    const uint64_t* px_offset;
    const uint32_t* bbox_w;
    const uint32_t* bbox_h;
    const uint32_t* bbox_d;
    const uint32_t* vmin;                  // LR::aux_min
    const uint32_t* vmax;                  // LR::aux_max
    int g;                                 // greyInfo: 0 none, > 0 matlab levels, < 0 radiomics bins
    uint32_t rows;                         // table rows of the call: the level bound + 1 (row = level)
    double soft_nan;
    double* out;                           // [n_roi of the BATCH x ld]
    uint64_t ld;
    int* status;
    const unsigned char* box;              // binned boxes of the chunk, box_stride bytes per ROI
    uint64_t box_stride;
    uint32_t max_cells;                    // what the strides were sized for
    uint32_t side_max[3];                  // largest w, h, d of the batch: what the grids were sized for
    uint32_t pitch_max;                    // largest vdz_pitch(w, h) of the batch: what tab_stride was sized for
    uint32_t* tab;                         // tables of the chunk, tab_stride words per ROI (zeroed by the caller)
    uint64_t tab_stride;
    uint16_t* dist;                        // the distance map, a value per cell, dist_stride values per ROI
    uint64_t dist_stride;
    uint32_t* label;                       // a label per cell, cell_stride words per ROI
    uint32_t* zmin;                        // the smallest distance per root, cell_stride words per ROI
    uint64_t cell_stride;
};

// the launches of the chain one by one: 0 distances along y, 1 distances along x, 2 init, 3 merge, 4 minimum, 5 emit, 6 close
constexpr int kVdzSteps = 7;
// Every function enqueues on `stream` and returns a hipError_t as int.
int launch_voldzone_step(const VoldzoneArgs& a, int step, void* stream);
int launch_voldzone(const VoldzoneArgs& a, void* stream);   // the whole chain from the binned boxes to the 18 columns

} // namespace nyxhip
