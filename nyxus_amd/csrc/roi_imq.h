// roi_imq.h -- host/device interface of the image-quality unit (roi_imq.hip): FOCUS_SCORE, LOCAL_FOCUS_SCORE, MAX_SATURATION and
// MIN_SATURATION of the reference's FeatureIMQ.  A header of its own, like roi_ih.h and roi_neighbors.h.  The class claims no family
// bit: its table [n_roi x kImqCols] belongs to the entries nyxhip_imq_batch / _tiles / _slides (nyxhip_imq.hip, nyxhip_tiles.hip).
#pragma once
#include <stdint.h>

namespace nyxhip {

constexpr int kImqCols = 4;                // FOCUS_SCORE, LOCAL_FOCUS_SCORE, MAX_SATURATION, MIN_SATURATION (featureset.h:920-931)
constexpr int kImqWaves = 4;               // wave form: ROIs (waves) per workgroup; workgroup forms: waves that share one ROI
// THE SWITCH-OVERS, by the cells w * h of the ROI's box (never by what else shares the launch):
//   cells <= kImqWaveCells                a wave per ROI, the plane in the wave's 4 KiB of LDS
//   cells <= kImqLdsCells                 a workgroup per ROI, the plane in 60 KiB of LDS
//   beyond                                a workgroup per ROI over a plane in a global workspace (classifier + list launch)
constexpr uint32_t kImqWaveCells = 1024;
constexpr uint32_t kImqLdsCells = 15360;
// whole slides: a workgroup takes kImqStripRows rows x kImqStripCols columns of a slide, halo cells read from the image itself
constexpr uint32_t kImqStripRows = 32;
constexpr uint32_t kImqStripCols = 256;
constexpr uint32_t kImqRowsAhead = 8;      // rows whose loads a thread of the slide kernel issues before it consumes the first (divides kImqStripRows)
// Regions whose Laplacian is summed: the box, then the (at most four) tiles of LOCAL_FOCUS_SCORE in the reference's loop order.
constexpr int kImqRegions = 5;
// One record of exact integer sums, 64-bit words: [0 .. 5) sum of L per region (two's complement) | [5 .. 15) sum of L^2 per region as
// (low, high) | [15] cloud pixels == max_inten | [16] == min_inten | [17] == 0.  Records add word by word (the pairs with carry).
constexpr int kImqWords = 18;

struct ImqArgs {
    uint64_t n_roi;
    const uint64_t* px_offset;             // [n_roi + 1]
    const uint16_t* x;
    const uint16_t* y;
    const uint32_t* inten;
    const uint32_t* bbox_w;
    const uint32_t* bbox_h;
    const uint32_t* vmin;                  // [n_roi] LR::aux_min
    const uint32_t* vmax;                  // [n_roi] LR::aux_max
    double soft_nan;
    double* out;                           // [n_roi x ld], the class's own table
    uint64_t ld;
    int* status;
    const uint32_t* roi_index;             // NULL: the LDS forms over every ROI; else workgroup b serves ROI roi_index[b] on a global plane
    uint32_t* ws;                          // list launches: ws_stride words of global plane per workgroup
    uint64_t ws_stride;
};

// wave_form / block_form: which of the two LDS launches to enqueue (each skips the ROIs of the other and the ROIs beyond LDS).
// block_cells: the largest box the workgroup form must hold (sizes its dynamic LDS; <= kImqLdsCells).  Returns a hipError_t as int.
int launch_roi_imq(const ImqArgs& a, void* stream, bool wave_form, bool block_form, uint32_t block_cells);
// the list launch: `count` workgroups over a.roi_index, planes in a.ws
int launch_roi_imq_list(const ImqArgs& a, void* stream, uint32_t count);
// predicate of the deferred list (deferred_list.h): ROIs with pixels whose box exceeds `cap` cells; hdr[1] = the most cells among them
struct ImqListed { const uint64_t* off; const uint32_t *bw, *bh; uint32_t cap; __device__ bool operator()(uint64_t i, uint32_t* hdr) const; };

// Whole slides: n_slides images of w x h elements of dt (NYXHIP_U8 / U16 / U32) back to back at `img`; vmin / vmax [n_slides] are the
// slides' extrema (roi_slide.hip).  `partials` holds imq_slide_records(w, h) records per slide.  Row t -> out + t * ld.
uint64_t imq_slide_records(uint32_t w, uint32_t h);
int launch_imq_slides(const void* img, int dt, uint32_t w, uint32_t h, uint32_t n_slides, const uint32_t* vmin, const uint32_t* vmax, uint64_t* partials,
                      double soft_nan, double* out, uint64_t ld, int* status, void* stream);

} // namespace nyxhip
