// roi_chords.h -- host/device interface of the chords kernel (roi_chords.hip): MAXCHORDS_* and ALLCHORDS_*.
// A header of its own, like roi_radial.h, roi_outline.h and roi_caliper.h.
#pragma once
#include "roi_kernel.h"

namespace nyxhip {

constexpr int kChordsCols = 16;            // MAXCHORDS_{MAX,MAX_ANG,MIN,MIN_ANG,MEDIAN,MEAN,MODE,STDDEV}, then the same eight for ALLCHORDS
constexpr int kChordsAngles = 20;          // the iterations of `for (ang = 0; ang < M_PI; ang += M_PI / 20)` (chords.cpp:22-23)
constexpr int kChordsSide = 100;           // n_side_segments: planes of >= 200 columns are scanned every (width / 100)-th column
constexpr int kChordsMaxCols = 2 * kChordsSide - 1;   // columns scanned per angle at most (199: width 199 with step 1)
constexpr int kChordsMaxAll = kChordsAngles * kChordsMaxCols;   // all chords of an ROI at most (3980)
// THE SWITCH-OVER: an ROI whose bound on the rotated bit plane, chords_plane_words(w, h), exceeds this many 32-bit words (32 KiB of
// LDS) goes through a global plane (list launch).  So does an ROI with zero-intensity pixels (min_inten == 0), whatever its size:
// "the last pixel of the cloud decides a cell" needs a word per cell.
constexpr uint32_t kChordsLdsWords = 8192;
constexpr uint32_t kChordsSortWords = 4096;   // the dynamic LDS is never smaller: the closing sorts <= 4000 chords through it

// Upper bound of either side of the tight box of a w x h box turned by any angle, the coordinates rounded to float and truncated:
// ceil(hypot(w, h)) + 2.
__host__ __device__ inline uint32_t chords_plane_side(uint32_t w, uint32_t h)
{
    const uint64_t q = (uint64_t)w * w + (uint64_t)h * h;
    uint64_t r = (uint64_t)sqrt((double)q);
    while (r * r > q) r--;
    while ((r + 1) * (r + 1) <= q) r++;
    return (uint32_t)(r + (r * r < q ? 1u : 0u) + 2u);
}
// ... and of the words of its column-major bit plane (every column padded to whole words)
__host__ __device__ inline uint64_t chords_plane_words(uint32_t w, uint32_t h)
{
    const uint64_t s = chords_plane_side(w, h);
    return s * ((s + 31u) / 32u);
}

struct ChordArgs {
    uint64_t n_roi;
    const uint64_t* px_offset;
    const uint16_t* x;
    const uint16_t* y;
    const uint32_t* inten;
    const uint32_t* bbox_w;
    const uint32_t* bbox_h;
    const uint32_t* min_inten;
    const uint32_t* origin_x;  // [n_roi] aabb.xmin / aabb.ymin of the ROI in its image, or NULL: (0, 0)
    const uint32_t* origin_y;
    double* out;
    uint64_t ld;
    int* status;
    int32_t col0;              // first of the 16 columns inside the output row
    uint32_t lds_words;        // words of the bit plane behind the kernel's dynamic LDS (<= kChordsLdsWords)
    const uint32_t* roi_index; // NULL: workgroup b serves ROI b and skips the ROIs of the list; else ROI roi_index[b], on global planes
    uint32_t* ws;              // list launches: (ws_words + ws_cells) words of global scratch per workgroup: bit plane | last-writer plane
    uint64_t ws_words, ws_cells;
    // the angles, and sin / cos of each as the reference takes them (rotation.cpp:70-82: the angle passed as float), filled on the host
    // through the host's libm
    double ang[kChordsAngles], sn[kChordsAngles], cs[kChordsAngles];
};

int launch_roi_chords(const ChordArgs& a, void* stream, uint32_t grid);
// predicate of the deferred list (deferred_list.h): the ROIs of the list launch; hdr[1] = largest chords_plane_words among them
// (saturated), hdr[2] = largest chords_plane_side among those with min_inten == 0
struct ChordsListed { const uint32_t *bw, *bh, *min_inten; uint32_t lds_words; __device__ bool operator()(uint64_t i, uint32_t* hdr) const; };

} // namespace nyxhip
