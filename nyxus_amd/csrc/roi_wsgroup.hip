// roi_wsgroup.hip -- whole-slide mode of three classes of the reference's *WHOLESLIDE* group (gfx950): the slide is ONE ROI at origin
// (0, 0), zero pixels included, in row-major order, and its contour is the four corners K = (0,0), (w-1,0), (w-1,h-1), (0,h-1) with
// the slide's maximum as their intensity (features/contour.cpp:917-933 of the reference).
//   ContourFeature             contour.cpp:935-986 over K: closed forms of w, h and the maximum (ws_close_kernel)
//   Smoms2D / Imoms2D_feature  2d_geomoments_basic.cpp:58-134: the unweighted sets as on the batch path; the weight of a pixel in the first
//                              / last row or column is epsilon = 0.001 whatever its intensity, of every other pixel I * log(d + epsilon) with
//                              d = min(x, w-1-x, y, h-1-y) -- the reference's dist_to_segment to the four sides, exact because the operands
//                              are integers and the root is of a perfect square -- and I = 1 for the shape variant; through float, as
//                              the reference's vector<float>
//   RadialDistributionFeature  radial_distribution.cpp:43-105 against K: find_center by the reference's hill descent over four points
//                              (contour_descent.h; with n = 4 the first step is 2, so corners 0 and 2 decide whether 1 and 3 are looked at),
//                              the first pixel in row-major order wins ties; bins, wedges and tail of roi_radial.hip (radial_close.h)
//
// The image is read in place in its own element type.  A slide is cut into bands of whole rows (wsgroup_plan.h), a workgroup per band:
//   ws_sweep_kernel         moments + radial pass A.  A band travels through LDS in tiles of kTilePx pixels: 16-byte loads from the
//                           16-byte-aligned part of a tile, head and tail element by element, stored at the same offset modulo 16 -- and
//                           then thread k takes pixels k, k + 256, ... of the BAND, so which thread sums which pixel never depends on
//                           where the slide lies in memory.  One record of fp64 partial sums and one (max - min, index) key per band.
//   ws_close_kernel         a wave per slide: adds the records in band order, the closing math of moments_close.h, the contour block, the
//                           centre and its max_sqdist for pass B.
//   ws_radial_kernel        pass B: integer LDS counters per workgroup, flushed with integer atomics (the order cannot matter)
//   ws_radial_close_kernel  the tail, a lane per ring
// No floating-point atomics anywhere: a row has the same bits whatever shares its call, its chunk or its place in the stack.
// Built with -ffp-contract=off (device_math.h).
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_wsgroup.h"
#include "contour_descent.h"
#include "moments_close.h"
#include "radial_close.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

constexpr int kWB = 256;
constexpr uint32_t kTilePx = 1024;
constexpr int kWsStep0 = 2;                   // (int)(4 / log(4)): the first step of the hill descent over four points (pixel.cpp:47)

__device__ __forceinline__ uint64_t d2u(double v) { return (uint64_t)__double_as_longlong(v); }
__device__ __forceinline__ double u2d(uint64_t v) { return __longlong_as_double((long long)v); }

// cnt elements from src into LDS; returns where element 0 lies.  s_raw: kTilePx * sizeof(E) + 16 bytes, 16-byte aligned.  The caller
// synchronises before it reads.
template <typename E>
__device__ __forceinline__ const E* stage_tile(const E* __restrict__ src, uint32_t cnt, unsigned char* s_raw, uint32_t tid)
{
    constexpr uint32_t EPV = 16 / sizeof(E);                                  // elements of a 16-byte load
    const uint32_t a = (uint32_t)((uintptr_t)src & 15u);
    const bool elem_aligned = (a % sizeof(E)) == 0;                           // (a base off its element size: everything element by element)
    E* const d = (E*)(s_raw + (elem_aligned ? a : 0u));
    uint32_t head = elem_aligned ? ((16u - a) & 15u) / (uint32_t)sizeof(E) : cnt;
    if (head > cnt) head = cnt;
    const uint32_t nv = (cnt - head) / EPV, e1 = head + nv * EPV;
    const uint4* const v = (const uint4*)(src + head);
    uint4* const dv = (uint4*)(d + head);
    for (uint32_t i = tid; i < nv; i += kWB) dv[i] = v[i];
    for (uint32_t i = tid; i < head; i += kWB) d[i] = src[i];
    for (uint32_t i = e1 + tid; i < cnt; i += kWB) d[i] = src[i];
    return d;
}

// Sums N <= 16 doubles across the workgroup in a fixed order; total k goes to dst[k] as its bits.
template <int N>
__device__ __forceinline__ void ws_block_sum(const double (&v)[N], double* s_red, uint64_t* dst, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    double t[16];
#pragma unroll
    for (int k = 0; k < 16; k++) t[k] = k < N ? v[k] : 0.0;
    const double tot = wave_transpose_sum16(t, lane);
    if ((lane & 3) == 0 && (lane >> 2) < N) s_red[wave * 16 + (lane >> 2)] = tot;
    __syncthreads();
    if (tid < N) dst[tid] = d2u(((s_red[tid] + s_red[16 + tid]) + s_red[32 + tid]) + s_red[48 + tid]);
    __syncthreads();
}

__device__ __forceinline__ void corners(uint32_t* s_K, uint32_t w, uint32_t h)
{
    s_K[0] = 0u; s_K[1] = w - 1u; s_K[2] = (w - 1u) | ((h - 1u) << 16); s_K[3] = (h - 1u) << 16;   // tl, tr, br, bl (contour.cpp:926-930)
}

// grid (bands, slides)
template <typename E, bool SMALL>
__global__ __launch_bounds__(kWB) void ws_sweep_kernel(const E* __restrict__ img, uint32_t w, uint32_t h, uint32_t band_rows, uint32_t ws_mask,
                                                       uint64_t* __restrict__ partials)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[kTilePx * sizeof(E) + 16];
    __shared__ uint32_t s_K[4];
    __shared__ double s_red[4 * 16];
    __shared__ unsigned long long s_bd[4];
    __shared__ uint32_t s_bi[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t t = blockIdx.y, band = blockIdx.x;
    const E* const p = img + (uint64_t)t * w * h;
    const uint32_t y0 = band * band_rows, y1 = y0 + band_rows < h ? y0 + band_rows : h;
    const uint32_t i0 = y0 * w, i1 = y1 * w;                                  // (w * h < 2^32: sides are at most 65534)
    const bool do_i = (ws_mask & NYXHIP_WS_IMOMS) != 0, do_m = (ws_mask & (NYXHIP_WS_SMOMS | NYXHIP_WS_IMOMS)) != 0,
               do_r = (ws_mask & NYXHIP_WS_RADIAL) != 0;
    if (tid == 0) corners(s_K, w, h);
    const double obx = 0.5 * (double)(w - 1u), oby = 0.5 * (double)(h - 1u);  // sums about the box centre, as roi_moments.hip
    const double w_edge = (double)(float)0.001;                               // realintens[i] = epsilon, a float (pixel.h:8)
    double aI[16], wS[10], wI[10];
#pragma unroll
    for (int k = 0; k < 16; k++) aI[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 10; k++) { wS[k] = 0.0; wI[k] = 0.0; }
    unsigned long long bd = ~0ull;
    uint32_t bi = 0xFFFFFFFFu;
    const uint32_t dxs = (uint32_t)kWB % w, dys = (uint32_t)kWB / w;
    for (uint32_t b0 = i0; b0 < i1; b0 += kTilePx) {
        const uint32_t cnt = i1 - b0 < kTilePx ? i1 - b0 : kTilePx;
        const E* const d = stage_tile<E>(p + b0, cnt, s_raw, (uint32_t)tid);
        __syncthreads();
        uint32_t idx = b0 + (uint32_t)tid;
        uint32_t y = idx / w, x = idx - y * w;
        for (uint32_t k = (uint32_t)tid; k < cnt; k += kWB) {
            const uint32_t v = (uint32_t)d[k];
            if (do_m) {
                const double X = (double)x - obx, Y = (double)y - oby, I = (double)v;
                const double yp[4] = {1.0, Y, Y * Y, Y * Y * Y};
                // aligned() with a corner: the first / last row or column.  Every other pixel: the least distance to a side.
                const bool edge = x == 0u || y == 0u || x == w - 1u || y == h - 1u;
                const uint32_t dmx = x < w - 1u - x ? x : w - 1u - x, dmy = y < h - 1u - y ? y : h - 1u - y;
                const double lg = log((double)(dmx < dmy ? dmx : dmy) + 0.001);
                const double Ws = edge ? w_edge : (double)(float)(1.0 * lg), Wi = edge ? w_edge : (double)(float)(I * lg);
                double xpw = 1.0;
#pragma unroll
                for (int pp = 0; pp < 4; pp++) {
                    if (pp) xpw = pp == 1 ? X : xpw * X;                      // X, X * X, (X * X) * X
                    if (do_i) {
                        const double ix = pp ? I * xpw : I;
#pragma unroll
                        for (int q = 0; q < 4; q++) aI[pp * 4 + q] = q ? __builtin_fma(ix, yp[q], aI[pp * 4 + q]) : aI[pp * 4 + q] + ix;
                    }
                    const double sx = pp ? Ws * xpw : Ws, ixv = pp ? Wi * xpw : Wi;
#pragma unroll
                    for (int k2 = 0; k2 < 10; k2++)
                        if (MomPQ::wr_p[k2] == pp) {
                            wS[k2] = MomPQ::wr_q[k2] ? __builtin_fma(sx, yp[MomPQ::wr_q[k2]], wS[k2]) : wS[k2] + sx;
                            wI[k2] = MomPQ::wr_q[k2] ? __builtin_fma(ixv, yp[MomPQ::wr_q[k2]], wI[k2]) : wI[k2] + ixv;
                        }
                }
            }
            if (do_r) {
                // find_center (pixel.cpp:146-162): max - min is an integer below 2^35; the first pixel of the row-major order wins a tie
                const double mn = sqdist_descent<SMALL, false>((int)x, (int)y, s_K, 4, kWsStep0, nullptr, 0),
                             mx = sqdist_descent<SMALL, true>((int)x, (int)y, s_K, 4, kWsStep0, nullptr, 0);
                const unsigned long long dif = (unsigned long long)(mx - mn);  // (both descents start at K[0]: mn <= mx)
                if (dif < bd || (dif == bd && idx < bi)) { bd = dif; bi = idx; }
            }
            idx += kWB; x += dxs; y += dys;
            if (x >= w) { x -= w; y++; }
        }
        __syncthreads();
    }
    uint64_t* const rec = partials + ((uint64_t)t * gridDim.x + band) * kWsWords;
    ws_block_sum<16>(aI, s_red, rec, tid);
    ws_block_sum<10>(wS, s_red, rec + 16, tid);
    ws_block_sum<10>(wI, s_red, rec + 26, tid);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long od = __shfl_xor(bd, o, 64);
        const uint32_t oi = __shfl_xor(bi, o, 64);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    if (lane == 0) { s_bd[wave] = bd; s_bi[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; k++)
            if (s_bd[k] < bd || (s_bd[k] == bd && s_bi[k] < bi)) { bd = s_bd[k]; bi = s_bi[k]; }
        rec[36] = bd; rec[37] = bi;
    }
}

struct WsCloseArgs {
    uint32_t w, h, bands, ws_mask;
    const uint32_t* vmax;
    const uint64_t* partials;
    uint64_t* centre;
    double* out;
    uint64_t ld;
    int32_t col_contour, col_smoms, col_imoms;
};

// grid (slides), one wave
__global__ __launch_bounds__(64) void ws_close_kernel(const WsCloseArgs A)
{
    __shared__ double s_mo[2][16], s_wo16[2][16], s_raw[2][16], s_cen[2][16], s_wraw[2][10], s_wcen[2][7], s_ax[2][4];
    __shared__ uint32_t s_K[4];
    const int lane = threadIdx.x;
    const uint32_t t = blockIdx.x, w = A.w, h = A.h;
    double* const row = A.out + (uint64_t)t * A.ld;
    const uint64_t* const recs = A.partials + (uint64_t)t * A.bands * kWsWords;
    const bool do_c = (A.ws_mask & NYXHIP_WS_CONTOUR) != 0, do_s = (A.ws_mask & NYXHIP_WS_SMOMS) != 0, do_i = (A.ws_mask & NYXHIP_WS_IMOMS) != 0,
               do_r = (A.ws_mask & NYXHIP_WS_RADIAL) != 0;
    if (lane == 0) corners(s_K, w, h);
    __syncthreads();
    // ---- ContourFeature::calculate over the four corners (contour.cpp:959-985): the perimeter closes K[3] -> K[0] first; four equal
    //      intensities leave Moments4 with mean = the value and M2 = 0
    if (do_c && lane == 0) {
        const double sw = (double)(w - 1u), sh = (double)(h - 1u), v = (double)A.vmax[t];
        double per = 0.0;
        per += sqrt(sh * sh); per += sqrt(sw * sw); per += sqrt(sh * sh); per += sqrt(sw * sw);
        double* const o = row + A.col_contour;
        o[0] = per; o[1] = per / 3.14159265358979323846; o[2] = v; o[3] = 0.0; o[4] = v; o[5] = v; o[6] = ((v + v) + v) + v;
    }
    if (do_s || do_i) {
        const double obx = 0.5 * (double)(w - 1u), oby = 0.5 * (double)(h - 1u);
        // the records in band order: lane k owns word k
        double acc = 0.0;
        if (lane < 36)
            for (uint32_t b = 0; b < A.bands; b++) acc += u2d(recs[(uint64_t)b * kWsWords + lane]);
        if (lane < 32) s_wo16[lane >> 4][lane & 15] = 0.0;       // the ten sums in the [p * 4 + q] layout of mom_shifted (the other six: zero)
        if (lane < 16) s_mo[1][lane] = acc;
        // the shape variant's unweighted sums factor: sum_x (x - ox)^p times sum_y (y - oy)^q
        for (int ax = 0; ax < 2; ax++) {
            const uint32_t n = ax ? h : w;
            const double o = ax ? oby : obx;
            double a1 = 0.0, a2 = 0.0, a3 = 0.0;
            for (uint32_t i = (uint32_t)lane; i < n; i += 64) { const double dv = (double)i - o; a1 += dv; a2 += dv * dv; a3 += dv * dv * dv; }
            a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);
            if (lane == 0) { s_ax[ax][0] = (double)n; s_ax[ax][1] = a1; s_ax[ax][2] = a2; s_ax[ax][3] = a3; }
        }
        __syncthreads();
        if (lane >= 16 && lane < 36) { const int var = (lane - 16) / 10, k = (lane - 16) % 10; s_wo16[var][MomPQ::wr_p[k] * 4 + MomPQ::wr_q[k]] = acc; }
        if (lane < 16) s_mo[0][lane] = s_ax[0][lane >> 2] * s_ax[1][lane & 3];
        __syncthreads();
        // from here on: roi_moments.hip's passes 2 and 4 (raw: origin 0; central: the centroid; each variant its own)
        if (lane < 32) { const int var = lane >> 4, pq = lane & 15; s_raw[var][pq] = mom_shifted(s_mo[var], pq >> 2, pq & 3, obx, oby); }
        __syncthreads();
        if (lane < 32) {
            const int var = lane >> 4, pq = lane & 15;
            const double cx = s_raw[var][4] / s_raw[var][0], cy = s_raw[var][1] / s_raw[var][0];
            s_cen[var][pq] = mom_shifted(s_mo[var], pq >> 2, pq & 3, obx - cx, oby - cy);
        }
        if (lane < 20) { const int var = lane / 10, k = lane % 10; s_wraw[var][k] = mom_shifted(s_wo16[var], MomPQ::wr_p[k], MomPQ::wr_q[k], obx, oby); }
        __syncthreads();
        if (lane < 14) {
            const int var = lane / 7, k = lane % 7;
            const double ox = s_wraw[var][4] / s_wraw[var][0], oy = s_wraw[var][1] / s_wraw[var][0];
            s_wcen[var][k] = mom_shifted(s_wo16[var], MomPQ::nc_p[k], MomPQ::nc_q[k], obx - ox, oby - oy);
        }
        __syncthreads();
        if (lane < 2 && (lane ? do_i : do_s))
            mom_write_block(row + (lane ? A.col_imoms : A.col_smoms), s_raw[lane], s_cen[lane], s_wraw[lane], s_wcen[lane]);
    }
    if (do_r) {
        unsigned long long bd = ~0ull;
        uint32_t bi = 0xFFFFFFFFu;
        for (uint32_t b = (uint32_t)lane; b < A.bands; b += 64) {
            const unsigned long long od = recs[(uint64_t)b * kWsWords + 36];
            const uint32_t oi = (uint32_t)recs[(uint64_t)b * kWsWords + 37];
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long od = __shfl_xor(bd, o, 64);
            const uint32_t oi = __shfl_xor(bi, o, 64);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
        if (lane == 0) {
            const uint32_t cy = bi / w, cx = bi - cy * w;                     // (every band has a pixel: bi < w * h)
            const bool small = w < 32768u && h < 32768u;
            const double c_mx = small ? sqdist_descent<true, true>((int)cx, (int)cy, s_K, 4, kWsStep0, nullptr, 0)
                                      : sqdist_descent<false, true>((int)cx, (int)cy, s_K, 4, kWsStep0, nullptr, 0);
            A.centre[(uint64_t)t * kWsCentreWords] = (uint64_t)cx | ((uint64_t)cy << 32);
            A.centre[(uint64_t)t * kWsCentreWords + 1] = d2u(c_mx);
        }
    }
}

// grid (bands, slides): pass B (radial_distribution.cpp:74-99)
template <typename E>
__global__ __launch_bounds__(kWB) void ws_radial_kernel(const E* __restrict__ img, uint32_t w, uint32_t h, uint32_t band_rows,
                                                        const uint64_t* __restrict__ centre, unsigned long long* __restrict__ bins, uint32_t wedge_tab)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[kTilePx * sizeof(E) + 16];
    __shared__ unsigned long long s_wedge[4][kRadialBins * kRadialBins];     // a replica per wave: LDS atomics of a wave meet only their own
    __shared__ uint32_t s_cnt[4][kRadialBins];
    const int tid = threadIdx.x, wave = tid >> 6;
    const uint32_t t = blockIdx.y, band = blockIdx.x;
    const uint64_t cxy = centre[(uint64_t)t * kWsCentreWords];
    const double c_mx = u2d(centre[(uint64_t)t * kWsCentreWords + 1]);
    if (!(c_mx > 0.0)) return;                                               // the undefined case (a 1 x 1 slide): 24 zeros, DESIGN.md 4.5a
    const int cx = (int)(uint32_t)cxy, cy = (int)(uint32_t)(cxy >> 32);
    const double dstOC = sqrt(c_mx);
    const E* const p = img + (uint64_t)t * w * h;
    const uint32_t y0 = band * band_rows, y1 = y0 + band_rows < h ? y0 + band_rows : h;
    const uint32_t i0 = y0 * w, i1 = y1 * w;
    for (int i = tid; i < 4 * kRadialBins * kRadialBins; i += kWB) (&s_wedge[0][0])[i] = 0ull;
    if (tid < 4 * kRadialBins) (&s_cnt[0][0])[tid] = 0u;
    const uint32_t dxs = (uint32_t)kWB % w, dys = (uint32_t)kWB / w;
    for (uint32_t b0 = i0; b0 < i1; b0 += kTilePx) {
        const uint32_t cnt = i1 - b0 < kTilePx ? i1 - b0 : kTilePx;
        const E* const d = stage_tile<E>(p + b0, cnt, s_raw, (uint32_t)tid);
        __syncthreads();
        const uint32_t idx = b0 + (uint32_t)tid;
        uint32_t y = idx / w, x = idx - y * w;
        for (uint32_t k = (uint32_t)tid; k < cnt; k += kWB) {
            const int dx = (int)x - cx, dy = (int)y - cy;
            const int ring = ring_of(dx, dy, dstOC);
            atomicAdd(&s_cnt[wave][ring], 1u);
            atomicAdd(&s_wedge[wave][ring * kRadialBins + wedge_of(dx, dy, wedge_tab)], (unsigned long long)(uint32_t)d[k]);
            x += dxs; y += dys;
            if (x >= w) { x -= w; y++; }
        }
        __syncthreads();
    }
    unsigned long long* const B = bins + (uint64_t)t * kWsBinWords;
    if (tid < kRadialBins * kRadialBins) {
        const unsigned long long s = ((s_wedge[0][tid] + s_wedge[1][tid]) + s_wedge[2][tid]) + s_wedge[3][tid];
        if (s) atomicAdd(&B[kRadialBins + tid], s);
    }
    if (tid < kRadialBins) {
        const uint32_t c = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
        if (c) atomicAdd(&B[tid], (unsigned long long)c);
    }
}

// grid (slides): get_FracAtD, get_MeanFrac, get_RadialCV (:212-247), a lane per ring
__global__ __launch_bounds__(64) void ws_radial_close_kernel(const uint64_t* __restrict__ centre, const unsigned long long* __restrict__ bins, uint32_t w, uint32_t h,
                                                             double* __restrict__ out, uint64_t ld, int32_t col)
{
    const uint32_t t = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid >= kRadialBins) return;
    double* const row = out + (uint64_t)t * ld + col;
    double frac = 0.0, mean_frac = 0.0, cv = 0.0;                            // calculate() returns with its zero-filled vectors
    if (u2d(centre[(uint64_t)t * kWsCentreWords + 1]) > 0.0) {
        const unsigned long long* const B = bins + (uint64_t)t * kWsBinWords;
        unsigned long long wsum[kRadialBins];
#pragma unroll
        for (int k = 0; k < kRadialBins; k++) wsum[k] = B[kRadialBins + tid * kRadialBins + k];
        radial_tail((double)B[tid], wsum, (double)((uint64_t)w * h), frac, mean_frac, cv);
    }
    row[tid] = frac; row[kRadialBins + tid] = mean_frac; row[2 * kRadialBins + tid] = cv;
}

template <typename E>
int group(const WsArgs& a, hipStream_t st)
{
    const uint32_t rows = ws_band_rows(a.w), bands = ws_bands(a.w, a.h);
    const dim3 grid(bands, a.n_slides);
    const bool small = a.w < 32768u && a.h < 32768u;                          // squared distances exact in 32-bit integers (contour_descent.h)
    if (a.ws_mask & (NYXHIP_WS_SMOMS | NYXHIP_WS_IMOMS | NYXHIP_WS_RADIAL)) {
        if (small) hipLaunchKernelGGL((ws_sweep_kernel<E, true>), grid, dim3(kWB), 0, st, (const E*)a.img, a.w, a.h, rows, a.ws_mask, a.partials);
        else hipLaunchKernelGGL((ws_sweep_kernel<E, false>), grid, dim3(kWB), 0, st, (const E*)a.img, a.w, a.h, rows, a.ws_mask, a.partials);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    WsCloseArgs c{a.w, a.h, bands, a.ws_mask, a.vmax, a.partials, a.centre, a.out, a.ld, a.col_contour, a.col_smoms, a.col_imoms};
    hipLaunchKernelGGL(ws_close_kernel, dim3(a.n_slides), dim3(64), 0, st, c);
    if (int rc = (int)hipGetLastError()) return rc;
    if (a.ws_mask & NYXHIP_WS_RADIAL) {
        if (hipError_t e = hipMemsetAsync(a.bins, 0, 8ull * kWsBinWords * a.n_slides, st); e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(ws_radial_kernel<E>, grid, dim3(kWB), 0, st, (const E*)a.img, a.w, a.h, rows, (const uint64_t*)a.centre, (unsigned long long*)a.bins,
                           a.wedge_tab);
        if (int rc = (int)hipGetLastError()) return rc;
        hipLaunchKernelGGL(ws_radial_close_kernel, dim3(a.n_slides), dim3(64), 0, st, (const uint64_t*)a.centre, (const unsigned long long*)a.bins, a.w, a.h, a.out,
                           a.ld, a.col_radial);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}

} // namespace

int launch_wsgroup(const WsArgs& a, void* stream)
{
    if (a.n_slides == 0)
        return 0;
    hipStream_t st = (hipStream_t)stream;
    return a.dt == NYXHIP_U8 ? group<uint8_t>(a, st) : a.dt == NYXHIP_U16 ? group<uint16_t>(a, st) : group<uint32_t>(a, st);
}

} // namespace nyxhip
