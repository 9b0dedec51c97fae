// roi_circle.h -- host/device interface of the circle / geodetic unit (roi_circle.hip): DIAMETER_MIN_ENCLOSING_CIRCLE,
// DIAMETER_CIRCUMSCRIBING_CIRCLE, DIAMETER_INSCRIBING_CIRCLE and GEODETIC_LENGTH, THICKNESS.  A header of its own, like roi_radial.h,
// roi_outline.h, roi_caliper.h, roi_chords.h and roi_erosion.h.
#pragma once
#include "roi_kernel.h"

namespace nyxhip {

constexpr int kCirclesCols = 3;            // DIAMETER_MIN_ENCLOSING_CIRCLE, DIAMETER_CIRCUMSCRIBING_CIRCLE, DIAMETER_INSCRIBING_CIRCLE
constexpr int kGeodeticCols = 2;           // GEODETIC_LENGTH, THICKNESS
constexpr int kCircleWaves = 4;            // ROIs (waves) per workgroup of roi_circle_kernel

struct CircArgs {
    MomArgs m;                 // batch, contour workspace (ws_contour / n_contour), k_cap, plane_cap and launch filter of the contour launches
    uint32_t grid_rois;        // ROI slots of the launch (kCircleWaves per workgroup)
    uint32_t fams;             // subset of NYXHIP_FAM_CIRCLES | NYXHIP_FAM_GEODETIC
    int32_t col_circles;       // first of the 3 circle columns inside the output row
    int32_t col_geodetic;      // first of the 2 geodetic columns
    const uint32_t* origin_x;  // [n_roi] box origins (NULL: 0): the reference's contour points are padded + origin
    const uint32_t* origin_y;
};

int launch_roi_circle(const CircArgs& a, void* stream, uint32_t grid);

} // namespace nyxhip
