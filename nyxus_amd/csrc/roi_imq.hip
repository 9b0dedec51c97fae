// roi_imq.hip -- two image-quality classes of the reference on the device (gfx950):
//   FocusScoreFeature    FOCUS_SCORE, LOCAL_FOCUS_SCORE        features/focus_score.cpp:188-282 (of the reference)
//   SaturationFeature    MAX_SATURATION, MIN_SATURATION        features/saturation.cpp:74-95
// over the ROI's dense plane P (h rows, w columns: the intensity at every cloud pixel, 0 elsewhere -- LR::aux_image_matrix).
//
//   roi_imq_kernel<1, false>          a wave per ROI of at most kImqWaveCells cells, kImqWaves ROIs per workgroup; the plane in LDS
//   roi_imq_kernel<kImqWaves, false>  a workgroup per ROI of at most kImqLdsCells cells; the plane in LDS
//   roi_imq_kernel<kImqWaves, true>   a workgroup per listed ROI beyond that (deferred_list.h); the plane in a global workspace
//   imq_slide_kernel / imq_slide_close_kernel   whole slides: a workgroup per block of kImqStripRows x kImqStripCols cells reading the
//                                     image itself (halo included), one record of sums per workgroup, then a wave per slide adds them
//
// EVERY SUM IS AN EXACT INTEGER.  L = P[y-1][x] + P[y+1][x] + P[y][x-1] + P[y][x+1] - 4 P[y][x] (cells outside the region are 0) is an
// integer of at most 35 bits.  Per region (the box, and each tile of LOCAL_FOCUS_SCORE with zeros outside the TILE) a sweep collects
// S = sum L in 64 bits and Q = sum L^2 in 128 bits; the population variance is (n Q - S^2) / n^2, whose numerator is formed exactly in
// 128 bits and rounded to fp64 once.  Integer sums do not depend on the order of their terms, so a row has the same bits whichever
// kernel, launch geometry or neighbours served it -- the three regimes above and the slide path need no agreement on a summation
// order -- and the one sweep replaces the mean-then-deviations pair of sweeps of the reference, whose fp64 result this one agrees with
// to rounding (it is the exact value the reference's two roundings per cell approximate).
// Width: |S| <= 4 max_inten n and n Q <= (4 max_inten n)^2, so everything fits while 4 max_inten n < 2^63; an ROI beyond that bound is
// refused (status NYXHIP_ERR_UNSUPPORTED, NaN row), never wrapped.
// Built with -ffp-contract=off (device_math.h).
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_imq.h"
#include "deferred_list.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

struct Geo {
    uint32_t w, h;
    uint32_t M, N;             // tile rows / columns: h / 2, w / 2
    uint32_t nty, ntx;         // tiles visited along y / x: y0 in {0, M, ..} while y0 < h - M -> 1 (even side) or 2 (odd side); 0: side-1 box
    bool small;                // 4 * max_inten < 2^31: L^2 fits 64 bits
};

__device__ __forceinline__ Geo make_geo(uint32_t w, uint32_t h, uint32_t vmax)
{
    Geo G;
    G.w = w; G.h = h; G.M = h / 2u; G.N = w / 2u;
    const bool tiles = w >= 2u && h >= 2u;
    G.nty = tiles ? ((h & 1u) ? 2u : 1u) : 0u;
    G.ntx = tiles ? ((w & 1u) ? 2u : 1u) : 0u;
    G.small = vmax < (1u << 29);
    return G;
}

__device__ __forceinline__ void square(long long v, bool small, uint64_t& lo, uint64_t& hi)
{
    const uint64_t a = (uint64_t)(v < 0 ? -v : v);
    if (small) { lo = (uint64_t)(uint32_t)a * (uint64_t)(uint32_t)a; hi = 0; }
    else { lo = a * a; hi = __umul64hi(a, a); }
}

// R: one record (kImqWords words, roi_imq.h) in registers -- constant indices only.  The box term of one cell:
__device__ __forceinline__ void add_box(uint64_t* R, const Geo& G, uint32_t c, uint32_t u, uint32_t d, uint32_t l, uint32_t r)
{
    const long long L = (long long)u + (long long)d + (long long)l + (long long)r - 4ll * (long long)c;
    uint64_t lo, hi;
    square(L, G.small, lo, hi);
    R[0] += (uint64_t)L; R[5] += lo; R[6] += hi + (R[5] < lo ? 1u : 0u);
}

// the tile of a cell (at most one): 0 .. 3 = ty * 2 + tx, 4 = none
__device__ __forceinline__ uint32_t tile_of(const Geo& G, uint32_t y, uint32_t x)
{
    const uint32_t ty = (y >= G.M ? 1u : 0u) + (y >= 2u * G.M ? 1u : 0u), tx = (x >= G.N ? 1u : 0u) + (x >= 2u * G.N ? 1u : 0u);
    return ty < G.nty && tx < G.ntx ? ty * 2u + tx : 4u;
}

// the Laplacian of a cell of tile k (< 4) with zeros outside the tile
__device__ __forceinline__ long long tile_laplacian(const Geo& G, uint32_t k, uint32_t y, uint32_t x, uint32_t c, uint32_t u, uint32_t d, uint32_t l, uint32_t r)
{
    const uint32_t ly = y - (k >> 1) * G.M, lx = x - (k & 1u) * G.N;
    return (long long)(ly > 0u ? u : 0u) + (long long)(ly + 1u < G.M ? d : 0u) + (long long)(lx > 0u ? l : 0u) + (long long)(lx + 1u < G.N ? r : 0u) - 4ll * (long long)c;
}

// (S, lo, hi) into the sums of tile k; k == 4: nowhere
__device__ __forceinline__ void add_tile(uint64_t* R, uint32_t k, uint64_t S, uint64_t lo, uint64_t hi)
{
#pragma unroll
    for (uint32_t kk = 0; kk < 4; kk++) {
        const bool take = k == kk;
        const uint64_t tl = take ? lo : 0ull, th = take ? hi : 0ull;
        R[1 + kk] += take ? S : 0ull;
        R[7 + 2 * kk] += tl; R[8 + 2 * kk] += th + (R[7 + 2 * kk] < tl ? 1u : 0u);
    }
}

__device__ __forceinline__ void imq_cell(uint64_t* R, const Geo& G, uint32_t y, uint32_t x, uint32_t c, uint32_t u, uint32_t d, uint32_t l, uint32_t r)
{
    add_box(R, G, c, u, d, l, r);
    const uint32_t k = tile_of(G, y, x);
    const long long Lt = tile_laplacian(G, k & 3u, y, x, c, u, d, l, r);
    uint64_t lo, hi;
    square(Lt, G.small, lo, hi);
    add_tile(R, k, (uint64_t)Lt, lo, hi);
}

__device__ __forceinline__ void record_zero(uint64_t* R)
{
#pragma unroll
    for (int i = 0; i < kImqWords; i++) R[i] = 0;
}

// R += O, the (low, high) pairs with carry
__device__ __forceinline__ void record_add(uint64_t* R, const uint64_t* O)
{
#pragma unroll
    for (int i = 0; i < kImqRegions; i++) R[i] += O[i];
#pragma unroll
    for (int i = 0; i < kImqRegions; i++) {
        const uint64_t ol = O[5 + 2 * i], oh = O[6 + 2 * i];
        R[5 + 2 * i] += ol; R[6 + 2 * i] += oh + (R[5 + 2 * i] < ol ? 1u : 0u);
    }
#pragma unroll
    for (int i = 15; i < kImqWords; i++) R[i] += O[i];
}

__device__ __forceinline__ void record_wave_reduce(uint64_t* R)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        uint64_t O[kImqWords];
#pragma unroll
        for (int i = 0; i < kImqWords; i++) O[i] = (uint64_t)__shfl_xor((unsigned long long)R[i], o, 64);
        record_add(R, O);
    }
}

// hi * 2^64 + lo rounded to fp64 once (round to nearest even: the bits cut off are kept as a sticky bit)
__device__ __forceinline__ double u128_to_double(uint64_t lo, uint64_t hi)
{
    if (hi == 0) return (double)lo;
    const int lz = __clzll((long long)hi);
    uint64_t top = lz ? (hi << lz) | (lo >> (64 - lz)) : hi;
    const uint64_t rest = lz ? (lo << lz) : lo;
    if (rest) top |= 1ull;
    return (double)top * __longlong_as_double((long long)(1023 + 64 - lz) << 52);
}

// population variance of a region of `cells` cells from S = sum L and Q = sum L^2: (cells * Q - S^2) / cells^2
__device__ __forceinline__ double region_variance(uint64_t S, uint64_t ql, uint64_t qh, uint64_t cells)
{
    const long long s = (long long)S;
    const uint64_t a = (uint64_t)(s < 0 ? -s : s);
    const uint64_t nl = cells * ql, nh = __umul64hi(cells, ql) + cells * qh;
    const uint64_t sl = a * a, sh = __umul64hi(a, a);
    const uint64_t dl = nl - sl, dh = nh - sh - (nl < sl ? 1u : 0u);
    return u128_to_double(dl, dh) / ((double)cells * (double)cells);
}

// 4 * vmax * cells < 2^63 ?
__device__ __forceinline__ bool imq_fits(uint32_t vmax, uint64_t cells) { return (uint64_t)vmax * cells < (1ull << 61); }

// The four columns of one ROI from its record.  area: cloud pixels (> 0), cells = w * h (> 0).
__device__ __forceinline__ void imq_close(const uint64_t* R, const Geo& G, uint64_t area, uint32_t vmin, uint32_t vmax, double soft_nan, double* row)
{
    const uint64_t cells = (uint64_t)G.w * G.h;
    row[0] = region_variance(R[0], R[5], R[6], cells);
    if (G.nty == 0u)
        row[1] = soft_nan;                                                     // a side of 1: the reference's loop does not end
    else {
        const uint64_t tc = (uint64_t)G.M * G.N;
        double local = 0.0;
        for (uint32_t ty = 0; ty < G.nty; ty++)
            for (uint32_t tx = 0; tx < G.ntx; tx++) {
                const uint32_t k = ty * 2u + tx;
                // (k as a constant index: R lives in registers)
                const uint64_t S = k == 0 ? R[1] : k == 1 ? R[2] : k == 2 ? R[3] : R[4];
                const uint64_t ql = k == 0 ? R[7] : k == 1 ? R[9] : k == 2 ? R[11] : R[13];
                const uint64_t qh = k == 0 ? R[8] : k == 1 ? R[10] : k == 2 ? R[12] : R[14];
                local += region_variance(S, ql, qh, tc);
            }
        row[1] = local / 4.0;                                                  // / (scale * scale)
    }
    // saturation.cpp:74-95 over the plane: the background cells are zeros of the plane
    const uint64_t bg = cells > area ? cells - area : 0ull;
    const uint32_t pmin = bg ? 0u : vmin, pmax = vmax;
    const uint64_t n_max = R[15] + (vmax == 0u ? bg : 0ull);
    const uint64_t n_min = pmin == pmax ? 0ull : (bg ? R[17] + bg : R[16]);   // if (== max) .. else if (== min)
    row[2] = (double)n_max / (double)cells;
    row[3] = (double)n_min / (double)cells;
}

__device__ __forceinline__ void row_nan(double* row)
{
#pragma unroll
    for (int c = 0; c < kImqCols; c++) row[c] = __longlong_as_double(0x7ff8000000000000LL);
}

template <int TEAM, bool GS>
__global__ __launch_bounds__(64 * kImqWaves) void roi_imq_kernel(const ImqArgs A, uint32_t lds_cells)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t imq_lds[];
    __shared__ uint64_t s_part[kImqWaves][kImqWords];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t roi;
    if (GS) roi = A.roi_index[blockIdx.x];
    else roi = TEAM == 1 ? (uint64_t)blockIdx.x * kImqWaves + (uint64_t)wave : (uint64_t)blockIdx.x;
    if (roi >= A.n_roi)
        return;
    const uint64_t off = A.px_offset[roi];
    const uint64_t npx = A.px_offset[roi + 1] - off;
    const uint32_t w = A.bbox_w[roi], h = A.bbox_h[roi];
    const uint64_t cells = (uint64_t)w * h;
    const bool empty = npx == 0 || cells == 0;
    // every ROI belongs to exactly one form, by its box alone (uniform over the team)
    const bool wave_roi = empty || cells <= kImqWaveCells, lds_roi = !wave_roi && cells <= kImqLdsCells;
    if (GS ? (wave_roi || lds_roi) : TEAM == 1 ? !wave_roi : !lds_roi)
        return;
    double* const row = A.out + roi * A.ld;
    const uint32_t tid = TEAM == 1 ? (uint32_t)lane : threadIdx.x;
    constexpr uint32_t T = 64u * TEAM;
    if (empty) {
        if (tid < (uint32_t)kImqCols) row[tid] = A.soft_nan;
        return;
    }
    const uint32_t vmn = A.vmin[roi], vmx = A.vmax[roi];
    if (!imq_fits(vmx, cells)) {                                               // the 64-bit sum of L could wrap: refused, not wrapped
        if (tid == 0) { atomicCAS(A.status, 0, NYXHIP_ERR_UNSUPPORTED); row_nan(row); }
        return;
    }
    if (GS ? (cells > A.ws_stride || cells > 0xFFFFFFFFull) : (TEAM != 1 && cells > lds_cells)) {   // the stated extrema did not cover this box
        if (tid == 0) { atomicCAS(A.status, 0, NYXHIP_ERR_ROI_TOO_LARGE); row_nan(row); }
        return;
    }
    uint32_t* const P = GS ? A.ws + (uint64_t)blockIdx.x * A.ws_stride : imq_lds + (TEAM == 1 ? (size_t)wave * kImqWaveCells : (size_t)0);
    auto sync = [] { if (TEAM == 1) wav_sync<false>(); else blk_sync<GS>(); };
    for (uint64_t i = tid; i < cells; i += T) P[i] = 0u;
    sync();
    uint64_t R[kImqWords];
    record_zero(R);
    {
        const uint16_t* const X = A.x + off; const uint16_t* const Y = A.y + off; const uint32_t* const V = A.inten + off;
        bool bad = false;
        for (uint64_t i = tid; i < npx; i += T) {
            const uint32_t x = X[i], y = Y[i], v = V[i];
            if (x < w && y < h) P[(uint64_t)y * w + x] = v; else bad = true;
            R[15] += v == vmx ? 1u : 0u; R[16] += v == vmn ? 1u : 0u; R[17] += v == 0u ? 1u : 0u;
        }
        if (bad) atomicCAS(A.status, 0, NYXHIP_ERR_INVALID_ARG);               // a pixel outside its box (never stored)
    }
    sync();
    const Geo G = make_geo(w, h, vmx);
    {
        uint32_t x = tid % w, y = tid / w;
        const uint32_t dx = T % w, dy = T / w;
        for (uint64_t i = tid; i < cells; i += T) {
            const uint32_t c = P[i];
            const uint32_t u = y > 0u ? P[i - w] : 0u, d = y + 1u < h ? P[i + w] : 0u;
            const uint32_t l = x > 0u ? P[i - 1] : 0u, r = x + 1u < w ? P[i + 1] : 0u;
            imq_cell(R, G, y, x, c, u, d, l, r);
            x += dx; y += dy;
            if (x >= w) { x -= w; y++; }
        }
    }
    record_wave_reduce(R);
    if (TEAM != 1) {
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < kImqWords; i++) s_part[wave][i] = R[i];
        }
        __syncthreads();
        if (threadIdx.x != 0)
            return;
        for (int k = 1; k < kImqWaves; k++) {
            uint64_t O[kImqWords];
#pragma unroll
            for (int i = 0; i < kImqWords; i++) O[i] = s_part[k][i];
            record_add(R, O);
        }
    } else if (lane != 0)
        return;
    imq_close(R, G, npx, vmn, vmx, A.soft_nan, row);
}

// grid (column blocks, row strips, slides).  partials: [slides][gridDim.y * gridDim.x] records.
template <typename E>
__global__ __launch_bounds__(256) void imq_slide_kernel(const E* __restrict__ img, uint32_t w, uint32_t h, const uint32_t* __restrict__ vmin,
                                                        const uint32_t* __restrict__ vmax, uint64_t* __restrict__ partials)
{
    __shared__ uint64_t s_part[4][kImqWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t t = blockIdx.z;
    const E* const p = img + (uint64_t)t * w * h;
    const uint32_t vmn = vmin[t], vmx = vmax[t];
    const Geo G = make_geo(w, h, vmx);
    const uint32_t x = blockIdx.x * kImqStripCols + threadIdx.x;
    const uint32_t y0 = blockIdx.y * kImqStripRows, y1 = y0 + kImqStripRows < h ? y0 + kImqStripRows : h;
    uint64_t R[kImqWords];
    record_zero(R);
    if (x < w && y0 < h) {
        // A thread walks down one column.  Its cells change tile at most twice, so the tile sums gather in registers of their own and
        // reach the record when the tile changes (add_tile's four predicated adds per change, not per cell).  The three loads of a row
        // (the cell below, left, right) are issued kImqRowsAhead rows at a time from clamped, always valid addresses -- a halo value
        // that lies outside the image is replaced by 0 afterwards -- so a wave has 3 * kImqRowsAhead loads in flight, not 3.
        const uint32_t xl = x > 0u ? x - 1u : 0u, xr = x + 1u < w ? x + 1u : x;
        uint32_t u = y0 > 0u ? (uint32_t)p[(uint64_t)(y0 - 1u) * w + x] : 0u;
        uint32_t c = (uint32_t)p[(uint64_t)y0 * w + x];
        uint32_t cur = 4u;
        // 8- and 16-bit images: |L| < 2^19, so over the kImqStripRows cells of a thread sum L fits 32 bits and sum L^2 64 bits (2^38 a
        // cell): no carries in the loop, one multiply-add per square.  32-bit images: the sums of the batch kernels.
        int32_t bS = 0, nS = 0;
        uint64_t bQ = 0, nQ = 0;
        uint32_t n_max = 0, n_min = 0;
        uint64_t tS = 0, tl = 0, th = 0;
        auto cell = [&](uint32_t y, uint32_t d, uint32_t l, uint32_t r) {
            const uint32_t k = tile_of(G, y, x);
            if constexpr (sizeof(E) < 4) {
                const int32_t L = (int32_t)(u + d + l + r) - 4 * (int32_t)c;
                bS += L; bQ += (uint64_t)((int64_t)L * (int64_t)L);
                if (k != cur) { add_tile(R, cur, (uint64_t)(int64_t)nS, nQ, 0ull); cur = k; nS = 0; nQ = 0; }
                if (k < 4u) {
                    const int32_t Lt = (int32_t)tile_laplacian(G, k, y, x, c, u, d, l, r);
                    nS += Lt; nQ += (uint64_t)((int64_t)Lt * (int64_t)Lt);
                }
            } else {
                add_box(R, G, c, u, d, l, r);
                if (k != cur) { add_tile(R, cur, tS, tl, th); cur = k; tS = tl = th = 0; }
                if (k < 4u) {
                    const long long Lt = tile_laplacian(G, k, y, x, c, u, d, l, r);
                    uint64_t lo, hi;
                    square(Lt, G.small, lo, hi);
                    tS += (uint64_t)Lt; tl += lo; th += hi + (tl < lo ? 1u : 0u);
                }
            }
            n_max += c == vmx ? 1u : 0u; n_min += c == vmn ? 1u : 0u;
            u = c; c = d;
        };
        for (uint32_t yb = y0; yb < y1; yb += kImqRowsAhead) {
            uint32_t dv[kImqRowsAhead], lv[kImqRowsAhead], rv[kImqRowsAhead];
#pragma unroll
            for (uint32_t i = 0; i < kImqRowsAhead; i++) {
                const uint32_t y = yb + i, yy = y < h ? y : h - 1u, yd = y + 1u < h ? y + 1u : h - 1u;
                const E* const row = p + (uint64_t)yy * w;
                lv[i] = (uint32_t)row[xl]; rv[i] = (uint32_t)row[xr]; dv[i] = (uint32_t)p[(uint64_t)yd * w + x];
            }
#pragma unroll
            for (uint32_t i = 0; i < kImqRowsAhead; i++) {
                const uint32_t y = yb + i;
                if (y < y1) cell(y, y + 1u < h ? dv[i] : 0u, x > 0u ? lv[i] : 0u, x + 1u < w ? rv[i] : 0u);
            }
        }
        if constexpr (sizeof(E) < 4) {
            add_tile(R, cur, (uint64_t)(int64_t)nS, nQ, 0ull);
            R[0] = (uint64_t)(int64_t)bS; R[5] = bQ;
        } else
            add_tile(R, cur, tS, tl, th);
        R[15] = n_max; R[16] = n_min;                                          // ([17], the zeros of the cloud, is read for a box with background only)
    }
    record_wave_reduce(R);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kImqWords; i++) s_part[wave][i] = R[i];
    }
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (int k = 1; k < 4; k++) {
        uint64_t O[kImqWords];
#pragma unroll
        for (int i = 0; i < kImqWords; i++) O[i] = s_part[k][i];
        record_add(R, O);
    }
    const uint64_t recs = (uint64_t)gridDim.x * gridDim.y;
    uint64_t* const dst = partials + ((uint64_t)t * recs + (uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * kImqWords;
#pragma unroll
    for (int i = 0; i < kImqWords; i++) dst[i] = R[i];
}

// a wave per slide: the records of its workgroups (integer sums: any order), then the closing of the batch kernels
__global__ __launch_bounds__(64) void imq_slide_close_kernel(const uint64_t* __restrict__ partials, uint64_t recs, uint32_t w, uint32_t h,
                                                             const uint32_t* __restrict__ vmin, const uint32_t* __restrict__ vmax, double soft_nan,
                                                             double* __restrict__ out, uint64_t ld, int* status)
{
    const uint32_t t = blockIdx.x;
    const int lane = threadIdx.x;
    uint64_t R[kImqWords];
    record_zero(R);
    for (uint64_t j = lane; j < recs; j += 64) {
        const uint64_t* const src = partials + ((uint64_t)t * recs + j) * kImqWords;
        uint64_t O[kImqWords];
#pragma unroll
        for (int i = 0; i < kImqWords; i++) O[i] = src[i];
        record_add(R, O);
    }
    record_wave_reduce(R);
    if (lane != 0)
        return;
    double* const row = out + (uint64_t)t * ld;
    const uint64_t cells = (uint64_t)w * h;
    if (!imq_fits(vmax[t], cells)) {
        atomicCAS(status, 0, NYXHIP_ERR_UNSUPPORTED);
        row_nan(row);
        return;
    }
    imq_close(R, make_geo(w, h, vmax[t]), cells, vmin[t], vmax[t], soft_nan, row);
}

template <typename E>
int slides(const void* img, uint32_t w, uint32_t h, uint32_t n, const uint32_t* vmin, const uint32_t* vmax, uint64_t* partials, double soft_nan,
           double* out, uint64_t ld, int* status, hipStream_t st)
{
    const dim3 grid((w + kImqStripCols - 1) / kImqStripCols, (h + kImqStripRows - 1) / kImqStripRows, n);
    hipLaunchKernelGGL(imq_slide_kernel<E>, grid, dim3(256), 0, st, (const E*)img, w, h, vmin, vmax, partials);
    if (int rc = (int)hipGetLastError()) return rc;
    hipLaunchKernelGGL(imq_slide_close_kernel, dim3(n), dim3(64), 0, st, (const uint64_t*)partials, imq_slide_records(w, h), w, h, vmin, vmax, soft_nan, out,
                       ld, status);
    return (int)hipGetLastError();
}

} // namespace

__device__ bool ImqListed::operator()(uint64_t i, uint32_t* hdr) const
{
    const uint64_t cells = (uint64_t)bw[i] * bh[i];
    if (cells <= cap || off[i + 1] == off[i])
        return false;
    atomicMax(&hdr[1], cells > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cells);
    return true;
}
template int deferred_classify<ImqListed>(uint64_t, const ImqListed&, uint32_t*, hipStream_t);

int launch_roi_imq(const ImqArgs& a, void* stream, bool wave_form, bool block_form, uint32_t block_cells)
{
    if (a.n_roi == 0)
        return 0;
    if (wave_form) {
        hipLaunchKernelGGL((roi_imq_kernel<1, false>), dim3((uint32_t)((a.n_roi + kImqWaves - 1) / kImqWaves)), dim3(64 * kImqWaves),
                           (size_t)kImqWaves * 4u * kImqWaveCells, (hipStream_t)stream, a, kImqWaveCells);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    if (block_form) {
        const uint32_t cells = block_cells < kImqLdsCells ? (block_cells > kImqWaveCells ? block_cells : kImqWaveCells + 1u) : kImqLdsCells;
        hipLaunchKernelGGL((roi_imq_kernel<kImqWaves, false>), dim3((uint32_t)a.n_roi), dim3(64 * kImqWaves), (size_t)4u * cells, (hipStream_t)stream, a, cells);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}

int launch_roi_imq_list(const ImqArgs& a, void* stream, uint32_t count)
{
    if (count == 0)
        return 0;
    hipLaunchKernelGGL((roi_imq_kernel<kImqWaves, true>), dim3(count), dim3(64 * kImqWaves), 0, (hipStream_t)stream, a, 0u);
    return (int)hipGetLastError();
}

uint64_t imq_slide_records(uint32_t w, uint32_t h)
{
    return (uint64_t)((w + kImqStripCols - 1) / kImqStripCols) * ((h + kImqStripRows - 1) / kImqStripRows);
}

int launch_imq_slides(const void* img, int dt, uint32_t w, uint32_t h, uint32_t n_slides, const uint32_t* vmin, const uint32_t* vmax, uint64_t* partials,
                      double soft_nan, double* out, uint64_t ld, int* status, void* stream)
{
    if (n_slides == 0)
        return 0;
    hipStream_t st = (hipStream_t)stream;
    return dt == NYXHIP_U8 ? slides<uint8_t>(img, w, h, n_slides, vmin, vmax, partials, soft_nan, out, ld, status, st)
         : dt == NYXHIP_U16 ? slides<uint16_t>(img, w, h, n_slides, vmin, vmax, partials, soft_nan, out, ld, status, st)
                            : slides<uint32_t>(img, w, h, n_slides, vmin, vmax, partials, soft_nan, out, ld, status, st);
}

} // namespace nyxhip
