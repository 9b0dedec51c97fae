// roi_volshape.h -- host/device interface of the volume shape unit (roi_volshape.hip): the 14 shape codes of the reference's Feature3D
// enum (D3_SurfaceFeature, features/3d_surface.cpp).  The table belongs to nyxhip_featurize_volumes_shape (nyxhip_volshape.hip); the
// batch type and the box limits are those of roi_vol.h.
#pragma once
#include <stdint.h>
#include "roi_vol.h"

namespace nyxhip {

constexpr int kVshCols = 14;               // Feature3D AREA .. FLATNESS (featureset.h:678-693)
// Column order of a row: the enum's.
enum { VSH_AREA, VSH_AREA_2_VOLUME, VSH_COMPACTNESS1, VSH_COMPACTNESS2, VSH_MESH_VOLUME, VSH_SPHERICAL_DISPROPORTION, VSH_SPHERICITY, VSH_VOLUME_CONVEXHULL,
       VSH_VOXEL_VOLUME, VSH_MAJOR_AXIS_LEN, VSH_MINOR_AXIS_LEN, VSH_LEAST_AXIS_LEN, VSH_ELONGATION, VSH_FLATNESS };

// Per-ROI 64-bit words of the head: [0] the exposed faces, [1..3] sums of x, y, z, [4..9] sums of xx, yy, zz, xy, xz, yz (all exact:
// box-relative coordinates are below 2^16 and an ROI has at most 2^24 voxels, so a sum of products stays below 2^56), [10] 6 V of the hull
// as an int64, [11] the hull candidates of the ROI.
constexpr uint32_t kVshHead = 16;
enum { VSH_H_FACES = 0, VSH_H_SUM = 1, VSH_H_MOM = 4, VSH_H_HULL6V = 10, VSH_H_NCAND = 11 };

// THE SWITCH-OVER of the hull kernel, by the ROI's own candidate count C (never by what else shares the launch):
//   C <= kVshLdsCand   the candidates (8 B each), the visited set (vsh_table(C) keys of 8 B) and the edge stack (3 C edges of 8 B) live in LDS
//   beyond             all three live in the chunk workspace; the code is the same, the storage bases differ
// At the bound: 8 + 64 + 24 = 96 KiB of the 160 KiB a gfx950 workgroup may claim.  A launch whose boxes admit fewer candidates than the
// bound (cand_stride of the batch) claims LDS for that many only -- every ROI of it is then below the bound -- so that small ROIs share a CU.
constexpr uint32_t kVshLdsCand = 1024;
// keys of the visited set of C candidates: a hull of C vertices has at most 3 C - 6 edges, each marked once per direction; a power of
// two above 8 C keeps the load of the open-addressed table under 3/4
__host__ __device__ inline uint64_t vsh_table(uint64_t c)
{
    uint64_t t = 64;
    while (t < 8u * c) t <<= 1;
    return t;
}
// LDS bytes of the three for a launch that keeps up to lds_cand candidates there
__host__ __device__ inline uint32_t vsh_lds_bytes(uint32_t lds_cand) { return 8u * lds_cand + 8u * (uint32_t)vsh_table(lds_cand) + 8u * 3u * lds_cand; }

struct VolshapeArgs {
    uint64_t roi0, n_roi;                  // the ROIs [roi0, roi0 + n_roi) of the batch: one chunk
    const uint64_t* px_offset;
    const uint16_t* x;
    const uint16_t* y;
    const uint16_t* z;
    const uint32_t* inten;
    const uint32_t* bbox_w;
    const uint32_t* bbox_h;
    const uint32_t* bbox_d;
    double soft_nan;
    double* out;                           // [n_roi of the BATCH x ld]
    uint64_t ld;
    int* status;
    uint32_t max_cells, max_px;            // what the strides were sized for
    uint32_t side_max[3];                  // largest w, h, d of the batch
    uint32_t rows_max;                     // largest count of (z, y) rows the strides hold: min(side_max[1] * side_max[2], max_cells)
    // the zeroed part of the workspace (one memset per chunk)
    unsigned long long* head;              // kVshHead words per ROI
    uint32_t* row_lo;                      // per (z, y) row 65536 - the smallest x of a voxel of non-zero intensity (0: none), row_stride words per ROI
    uint32_t* row_hi;                      // per row 1 + the largest such x (0: none)
    uint64_t row_stride;
    unsigned char* occ;                    // the occupancy box, a byte per cell: bit 0 a voxel, bit 1 a voxel of non-zero intensity
    uint64_t occ_stride;
    // the rest
    uint32_t* chain;                       // per plane z its two monotone chains, 2 h words (x | y << 16): 2 * row_stride words per ROI
    unsigned long long* cand;              // the candidates (x << 32 | y << 16 | z), cand_stride = 2 * row_stride per ROI
    uint64_t cand_stride;
    uint32_t lds_cand;                     // candidates the LDS of this launch holds: min(kVshLdsCand, cand_stride)
    unsigned long long* visited;           // the visited set beyond LDS: vsh_table(cand_stride) keys per ROI
    uint64_t visited_stride;
    unsigned long long* stack;             // the edge stack beyond LDS: 3 * cand_stride edges per ROI
    uint64_t stack_stride;
};

// the launches of the chain one by one: 0 occupancy, row extremes and moments, 1 exposed faces, 2 hull, 3 close
constexpr int kVshSteps = 4;
// Every function enqueues on `stream` and returns a hipError_t as int.
int launch_volshape_step(const VolshapeArgs& a, int step, void* stream);
int launch_volshape(const VolshapeArgs& a, void* stream);   // the whole chain from the cloud to the 14 columns

} // namespace nyxhip
