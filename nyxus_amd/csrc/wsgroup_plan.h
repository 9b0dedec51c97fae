// wsgroup_plan.h -- the host plan of nyxhip_wsgroup_slides (nyxhip_wsgroup.hip): how a slide is cut into bands of whole rows for the
// sweep kernels of roi_wsgroup.hip, what workspace a slide needs, and how many slides share a chunk under a device budget.  Plain C++
// (no HIP), like volscan_plan.h and features_plan.h, so that tests/cpp/test_wsgroup_plan.cpp exercises it on the host.
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace nyxhip {

// THE BAND CUT: a band is the largest number of WHOLE rows with at most WS_BAND_PIXELS pixels, and one row where a row alone is longer.
// Whole rows keep a band's pixels contiguous in memory, and the cut depends on the slide's shape alone -- never on what shares the
// call, the chunk or the stack -- so the per-band partial sums and their order of addition are a function of the slide.
constexpr uint32_t WS_BAND_PIXELS = 16384;
constexpr uint32_t kWsMaxSide = 65534;        // the batch ABI's coordinates are 16-bit (nyxhip_featurize_slides)

// One record of partial sums per band, 64-bit words:
//   [0 .. 16)   sum I (x - ox)^p (y - oy)^q, word p * 4 + q, about the box centre o (fp64)
//   [16 .. 26)  the ten weighted sums of the shape variant (MomPQ::wr_*), [26 .. 36) of the intensity variant (fp64)
//   [36], [37]  the band's least (max_sqdist - min_sqdist, pixel index) of find_center, as two unsigned words
constexpr int kWsWords = 38;
// Per slide: the centre pass A found (x | y << 32, then max_sqdist as fp64 bits), then pass B's integer bins: 8 ring counts, 8 x 8 wedge sums
constexpr int kWsCentreWords = 2;
constexpr int kWsBinWords = 8 + 64;
constexpr int kWsExtremaBytes = 64;           // the slide's share of the header arrays of launch_slide_headers (generous)

inline uint32_t ws_band_rows(uint32_t w)
{
    const uint32_t r = w ? WS_BAND_PIXELS / w : 0u;
    return r ? r : 1u;
}

inline uint32_t ws_bands(uint32_t w, uint32_t h)
{
    const uint32_t r = ws_band_rows(w);
    return (h + r - 1u) / r;
}

// device workspace of one slide, bytes (a multiple of 8)
inline uint64_t ws_workspace_bytes(uint32_t w, uint32_t h)
{
    return 8ull * ((uint64_t)kWsWords * ws_bands(w, h) + kWsCentreWords + kWsBinWords) + kWsExtremaBytes;
}

struct WsPlan {
    int ok;                    // 0: a side of 0 or beyond kWsMaxSide; -1: one slide and its workspace exceed the budget; 1: the rest is valid
    uint32_t band_rows, bands;
    uint64_t ws_bytes;         // workspace per slide
    uint64_t per_slide;        // device bytes a slide claims in a chunk: workspace + its output row + (host slides) two staging copies of the image
    uint64_t chunk;            // slides per chunk (>= 1, <= 65535: the kernels spend a grid dimension on the slides of a chunk)
    uint64_t n_chunks;         // ceil(n_slides / chunk); the last chunk holds n_slides - (n_chunks - 1) * chunk slides
};

// n_slides >= 1.  elem_bytes 1 / 2 / 4; n_cols: columns of the output row; host: the images are host memory (they travel through the
// double-buffered staging ring in copies of at most 512 MiB, at least two chunks from four slides on so that copy and sweep overlap).
inline WsPlan ws_plan(uint32_t w, uint32_t h, uint32_t elem_bytes, bool host, uint64_t n_slides, uint32_t n_cols, uint64_t budget)
{
    WsPlan p{};
    if (w == 0 || h == 0 || w > kWsMaxSide || h > kWsMaxSide) return p;
    p.band_rows = ws_band_rows(w);
    p.bands = ws_bands(w, h);
    p.ws_bytes = ws_workspace_bytes(w, h);
    const uint64_t in_bytes = (uint64_t)w * h * elem_bytes;
    p.per_slide = p.ws_bytes + 8ull * n_cols + (host ? 2 * in_bytes : 0);
    if (p.per_slide > budget) { p.ok = -1; return p; }
    uint64_t chunk = budget / p.per_slide;
    if (host) {
        const uint64_t cap = (512ull << 20) / in_bytes;
        if (chunk > (cap ? cap : 1)) chunk = cap ? cap : 1;
    }
    if (chunk > n_slides) chunk = n_slides;
    if (host && n_slides >= 4 && chunk > (n_slides + 1) / 2) chunk = (n_slides + 1) / 2;
    if (chunk > 65535) chunk = 65535;
    p.chunk = chunk;
    p.n_chunks = (n_slides + chunk - 1) / chunk;
    p.ok = 1;
    return p;
}

} // namespace nyxhip
