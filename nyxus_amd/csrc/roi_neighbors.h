// roi_neighbors.h -- host/device interface of the neighbor unit (roi_neighbors.hip): NUM_NEIGHBORS, PERCENT_TOUCHING,
// CLOSEST_NEIGHBOR{1,2}_{DIST,ANG}, ANG_BW_NEIGHBORS_{MEAN,STDDEV,MODE}.  A header of its own, like roi_circle.h.  Unlike every other
// unit this one is no per-ROI reduction: it relates the ROIs of one image to each other, so it has entries (nyxhip_neighbors_batch /
// _tiles) and an output table [n_roi x kNeighborCols] of its own and claims no family bit.
#pragma once
#include "roi_kernel.h"

namespace nyxhip {

constexpr int kNeighborCols = 9;           // NUM_NEIGHBORS .. ANG_BW_NEIGHBORS_MODE, enum order (featureset.h:162-171 of the reference)
constexpr int kNbThreads = 256;            // workgroup of roi_neighbors_narrow_kernel: one ROI
constexpr int kNbPointsPerLane = 4;        // contour points of the ROI a lane holds per pass (a pass: kNbThreads * kNbPointsPerLane points)
constexpr int kNbTile = 1024;              // contour points of a candidate per LDS tile (int2: 8 KiB)
constexpr int kNbMaxDistance = 46340;      // largest pixel_distance served: beyond it the reference's `radius * radius` overflows its int

struct NbArgs {
    uint64_t n_roi;
    const uint64_t* px_offset;
    const uint16_t* x;
    const uint16_t* y;
    const uint32_t* bbox_w;
    const uint32_t* bbox_h;
    const uint32_t* label;         // [n_roi] strictly ascending inside an image (checked by the geometry kernel through `status`)
    const uint32_t* origin_x;      // [n_roi] box origins in the image (NULL: 0)
    const uint32_t* origin_y;
    const uint64_t* image_offset;  // [n_images + 1] CSR over the rows, or NULL
    uint64_t n_images;
    const uint32_t* image_id;      // [n_roi] ascending image index per row (the tile path's TileRows::tile), or NULL; both NULL: one image
    const uint32_t* ws_contour;    // the contour chain's workspace (MomArgs::ws_contour / n_contour)
    const uint32_t* n_contour;
    int64_t radius;                // pixel_distance (1 .. kNbMaxDistance)
    // geometry table, a lane per ROI
    long long* box;                // [4 n_roi] xmin, xmax, ymin, ymax in image coordinates
    double* cen;                   // [2 n_roi] CENTROID_X, CENTROID_Y
    uint32_t* img_lo;              // [n_roi] the rows [img_lo, img_hi) of the ROI's image
    uint32_t* img_hi;
    // candidate lists: count, exclusive scan, fill
    uint32_t* cand_count;          // [n_roi]
    uint64_t* cand_off;            // [n_roi + 1]
    uint32_t* cand;                // [total] rows j != i of the image whose boxes overlap at `radius`, ascending; both contours non-empty
    unsigned long long* cand_min;  // [total] min over both contours of the squared distance (the narrow-phase kernel)
    uint8_t* cand_flag;            // [total] 1: a neighbor
    uint16_t* cand_ang;            // [total] clamp(round(angle), 0, 360) of the flagged candidates (the closing kernel's scratch)
    double* out;                   // [n_roi x ld], kNeighborCols columns
    uint64_t ld;
    int* status;
};

int launch_nb_extrema(uint64_t n_roi, const uint64_t* px_offset, const uint32_t* bw, const uint32_t* bh, uint32_t* ext3, void* stream);
int launch_nb_geometry(const NbArgs& a, void* stream);
int launch_nb_candidates_count(const NbArgs& a, void* stream);    // cand_count, then cand_off (exclusive scan; cand_off[n_roi]: total)
int launch_nb_candidates_fill(const NbArgs& a, void* stream);
int launch_nb_narrow(const NbArgs& a, void* stream);
int launch_nb_close(const NbArgs& a, void* stream);

} // namespace nyxhip
