// roi_ih.h -- host/device interface of the IBSI intensity-histogram unit (roi_ih.hip): the 46 IH_* columns of the reference's
// IntensityHistogramFeatures.  A header of its own, like roi_circle.h and roi_neighbors.h.  The class claims no family bit: its table
// [n_roi x kIhCols] belongs to the entries nyxhip_ih_batch / nyxhip_ih_tiles (nyxhip_ih.hip, nyxhip_tiles.hip).
#pragma once
#include <stdint.h>

namespace nyxhip {

constexpr int kIhCols = 46;                // IH_MEAN_VAL .. IH_BIN_SIZE (featureset.h:584-637 of the reference)
constexpr int kIhMaxBins = 4096;           // N (= GREYDEPTH) the kernels serve: kIhWaves histograms of N uint32 counters fill 64 KiB of LDS
constexpr int kIhWaves = 4;                // wave form: ROIs (waves) per workgroup; workgroup form: waves that share one ROI
constexpr uint32_t kIhWavePx = 256;        // ROIs of at most this many pixels take the wave form

struct IhArgs {
    uint64_t n_roi;
    const uint64_t* px_offset;             // [n_roi + 1]
    const uint32_t* inten;                 // [n_px]
    const uint32_t* vmin;                  // [n_roi] LR::aux_min
    const uint32_t* vmax;                  // [n_roi] LR::aux_max
    int32_t n_bins;                        // N; < 2 gates the class (a negative grey depth lands here)
    int32_t ibsi;                          // 0 gates the class
    uint32_t wave_px;                      // ROIs of at most this many pixels belong to the wave form, the others to the workgroup form
    double soft_nan;
    double* out;                           // [n_roi x ld], the class's own table
    uint64_t ld;
};

// wave_form / block_form: which of the two launches to enqueue (each skips the ROIs of the other).  Returns a hipError_t as int.
int launch_roi_ih(const IhArgs& a, void* stream, bool wave_form, bool block_form);

} // namespace nyxhip
