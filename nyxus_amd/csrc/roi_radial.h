// roi_radial.h -- host/device interface of the radial intensity distribution kernel (roi_radial.hip).  A header of its own:
// roi_kernel.h is one of the sources the measured HBM traffic of the metric kernels is keyed on (bench.py, profiles/hbm_traffic.json),
// and this family touches none of them.
#pragma once
#include "roi_kernel.h"

namespace nyxhip {

constexpr int kRadialBins = 8;            // RadialDistributionFeature::num_bins (radial_distribution.h:36): rings and wedges
constexpr int kRadialCols = 3 * kRadialBins;   // FRAC_AT_D, MEAN_FRAC, RADIAL_CV

// reads the contour the contour kernel left in MomArgs::ws_contour
struct RadArgs {
    MomArgs m;                // batch, contour workspace, LDS carve (pixels | contour | step table) and launch filter of the moments launches
    int32_t col_frac, col_mean, col_cv;   // first column of each block inside the output row (GABOR sits between the first two)
    uint32_t wedge_tab;       // wedge bin of the eight axis / diagonal directions k * 45 degrees, four bits each: the reference expression
                              // int(atan2(dy, dx) [+ 2 pi] / (2 pi / 8)) evaluated by the host's libm (launch_contour_families)
};

int launch_roi_radial(const RadArgs& a, void* stream, uint32_t grid);

} // namespace nyxhip
