// roi_radial.hip -- radial intensity distribution (RadialDistributionFeature: FRAC_AT_D, MEAN_FRAC, RADIAL_CV; 3 x 8 columns),
// /root/reference/src/nyx/features/radial_distribution.cpp:43-105, :212-247.
//
//   roi_radial_kernel    One 256-thread workgroup per ROI, launched like roi_moments_kernel over the contour roi_contour_kernel left
//                        in the workspace (same LDS carve: pixels | contour | step table; same HBM fall-backs beyond it).
//                        Pass A  the centre, Pixel2::find_center (features/pixel.cpp:146-162): per pixel the two hill descents
//                                min_sqdist / max_sqdist over the ordered contour, then the workgroup's argmin of
//                                (max - min, pixel index) -- the FIRST pixel of the caller's order that attains the minimum.
//                        Pass B  every pixel into one of 8 rings (distance to the centre against the centre's max_sqdist) and one
//                                of 8 wedges (direction from the centre); counts and intensity sums are INTEGERS in LDS, so the
//                                result does not depend on scheduling or on the path that served the ROI.
//                        Tail    eight lanes form the three vectors with the reference's operation sequence in fp64.
//   Everything that decides a bin is exact: squared distances are integers; the ring index is sqrt, sqrt, divide, multiply,
//   truncate in fp64 (correctly rounded operations, no contraction: -ffp-contract=off); the wedge of a direction strictly inside
//   an octant is an integer comparison, and the eight directions ON an octant boundary (axes and diagonals) take the bin the
//   host's libm gives the reference expression (RadArgs::wedge_tab) -- there is no atan2 on the device.
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_radial.h"
#include "radial_close.h"
#include "launch_util.h"
#include "contour_descent.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

constexpr int kRB = 256;
constexpr int kRW = kRB / 64;                 // waves: one replica of the bin tables each (LDS atomics of a wave meet only their own)

} // namespace

__global__ __launch_bounds__(kRB) void roi_radial_kernel(const RadArgs R)
{
    const MomArgs& A = R.m;
    __shared__ unsigned long long s_wedge[kRW][kRadialBins * kRadialBins];   // banded_wedges[ring][wedge] (size_t in the reference)
    __shared__ uint32_t s_cnt[kRW][kRadialBins];                              // radial_count_bins
    __shared__ unsigned long long s_bd[kRW];
    __shared__ uint32_t s_bi[kRW];
    // staged pixels | contour | step table: the carve of the moments kernel (launch_contour_families sizes it from the batch extrema)
    extern __shared__ __attribute__((aligned(16))) unsigned char rad_lds[];
    uint2* const s_px = (uint2*)rad_lds;                                  // [A.px_cap]  x | y << 16, intensity
    uint32_t* const s_K = (uint32_t*)(rad_lds + 8u * A.px_cap);           // [A.k_cap]
    uint16_t* const s_step = (uint16_t*)(s_K + A.k_cap);                  // [A.step_cap]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t roi = A.sp.roi_index ? A.sp.roi_index[blockIdx.x] : blockIdx.x;   // (a list: the big boxes of a batch)
    if (roi >= A.n_roi)
        return;
    const uint64_t off = A.px_offset[roi];
    const uint32_t n = (uint32_t)(A.px_offset[roi + 1] - off);
    const uint32_t bw_ = A.bbox_w[roi], bh_ = A.bbox_h[roi];
    if (A.sp.defer_large && (bw_ + 2u) * (bh_ + 2u) > A.plane_cap)
        return;                                                           // served by the launch over the big-box list
    double* const row_out = A.out + roi * A.ld;
    auto write_zeros = [&]() {                                            // calculate() returns with its zero-filled vectors (:38-40, :55-56)
        if (tid < kRadialBins) { row_out[R.col_frac + tid] = 0.0; row_out[R.col_mean + tid] = 0.0; row_out[R.col_cv + tid] = 0.0; }
    };
    const int nK = n ? (int)A.n_contour[roi] : 0;
    if (n == 0 || nK == 0) { write_zeros(); return; }
    const bool small_xy = bw_ + 2u < 32768u && bh_ + 2u < 32768u;         // integer distances are exact (sqdist_descent)
    const uint32_t* K = A.ws_contour + off;
    const bool k_lds = nK <= (int)A.k_cap;
    if (k_lds) {
        for (int i = tid; i < nK; i += kRB) s_K[i] = K[i];
        K = s_K;
    }
    // window width -> step of the hill descent (first step from n, later ones from windows of at most two steps)
    const int step0 = __builtin_amdgcn_readfirstlane(nK >= 2 ? (int)((double)nK / log((double)nK)) : 1);
    const int tab_n = min((int)A.step_cap, 2 * step0 + 2);
    for (int m = 11 + tid; m < tab_n; m += kRB) s_step[m] = (uint16_t)(int)((double)m / log((double)m));
    const bool staged = n <= A.px_cap;
    if (staged)
        for_each_cloud_pixel<kRB>(A.inten + off, A.x + off, A.y + off, n, tid, [&](uint32_t i, uint32_t vi, uint32_t xi, uint32_t yi) {
            s_px[i] = make_uint2(xi | (yi << 16), vi);
        });
    for (int i = tid; i < kRW * kRadialBins * kRadialBins; i += kRB) (&s_wedge[0][0])[i] = 0ull;
    if (tid < kRW * kRadialBins) (&s_cnt[0][0])[tid] = 0u;
    __syncthreads();
    auto sweep = [&](auto&& body) {                      // body(i, intensity, x, y) for this thread's pixels i = tid, tid + 256, ...
        if (staged) {
            for (uint32_t i = (uint32_t)tid; i < n; i += kRB) {
                const uint2 q = s_px[i];
                body(i, q.y, q.x & 0xFFFFu, q.x >> 16);
            }
        } else
            for_each_cloud_pixel<kRB>(A.inten + off, A.x + off, A.y + off, n, tid, body);
    };
    // (the contour normally sits in LDS: passing the array itself -- not a pointer that may also be global -- keeps the descents'
    //  loads ds_read; pixels are box-relative, the contour is in the padded coordinates the reference keeps: the +1 cancels nowhere,
    //  as in the reference, where the contour is shifted by the padding against the pixels, contour.cpp:673-678)
    auto min_max = [&](int x, int y, double& mn, double& mx) {
        if (!small_xy) {
            mn = min_sqdist_v2<false>(x, y, K, nK, step0, s_step, tab_n); mx = max_sqdist_v2<false>(x, y, K, nK, step0, s_step, tab_n);
        } else if (k_lds) {
            mn = min_sqdist_v2<true>(x, y, s_K, nK, step0, s_step, tab_n); mx = max_sqdist_v2<true>(x, y, s_K, nK, step0, s_step, tab_n);
        } else {
            mn = min_sqdist_v2<true>(x, y, K, nK, step0, s_step, tab_n); mx = max_sqdist_v2<true>(x, y, K, nK, step0, s_step, tab_n);
        }
    };
    // ---- pass A: find_center (pixel.cpp:146-162).  max - min is an integer below 2^35; the key (dif, index) is ordered
    //      lexicographically, which is the packed key dif << 32 | index wherever that fits 64 bits: the lowest index wins a tie
    //      like the strict `<` of pixel.cpp:155 over pixels visited in order.
    unsigned long long bd = ~0ull;
    uint32_t bi = 0xFFFFFFFFu;
    sweep([&](uint32_t i, uint32_t, uint32_t xi, uint32_t yi) {
        double mn, mx;
        min_max((int)xi, (int)yi, mn, mx);
        const unsigned long long dif = (unsigned long long)(mx - mn);     // (both descents start at K[0]: mn <= mx)
        if (dif < bd || (dif == bd && i < bi)) { bd = dif; bi = i; }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long od = __shfl_xor(bd, o, 64);
        const uint32_t oi = __shfl_xor(bi, o, 64);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    if (lane == 0) { s_bd[wave] = bd; s_bi[wave] = bi; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kRW; w++) {
        const unsigned long long od = s_bd[w];
        const uint32_t oi = s_bi[w];
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    // (n >= 1: some thread saw a pixel, so bi < n here)
    const uint32_t cxy = staged ? s_px[bi].x : ((uint32_t)A.x[off + bi] | ((uint32_t)A.y[off + bi] << 16));
    const int cx = (int)(cxy & 0xFFFFu), cy = (int)(cxy >> 16);
    double c_mn, c_mx;
    min_max(cx, cy, c_mn, c_mx);
    // ---- the undefined case: a centre whose max_sqdist is 0 makes the reference divide by zero and convert NaN / infinity to int.
    //      Here such an ROI has no radial profile: 24 zeros, like an ROI without a contour.
    if (!(c_mx > 0.0)) { write_zeros(); return; }
    const double dstOC = sqrt(c_mx);                                      // :72
    // ---- pass B: rings and wedges (:74-99) ------------------------------------------------------------------------------
    sweep([&](uint32_t, uint32_t vi, uint32_t xi, uint32_t yi) {
        const int dx = (int)xi - cx, dy = (int)yi - cy;
        const int ring = ring_of(dx, dy, dstOC);
        const int wdg = wedge_of(dx, dy, R.wedge_tab);
        atomicAdd(&s_cnt[wave][ring], 1u);
        atomicAdd(&s_wedge[wave][ring * kRadialBins + wdg], (unsigned long long)vi);
    });
    __syncthreads();
    // ---- tail: get_FracAtD, get_MeanFrac, get_RadialCV (:212-247), one lane per ring ----------------------------------------
    if (tid < kRadialBins) {
        uint32_t cnt = 0;
        unsigned long long wsum[kRadialBins];
#pragma unroll
        for (int k = 0; k < kRadialBins; k++) wsum[k] = 0;
#pragma unroll
        for (int w = 0; w < kRW; w++) {
            cnt += s_cnt[w][tid];
#pragma unroll
            for (int k = 0; k < kRadialBins; k++) wsum[k] += s_wedge[w][tid * kRadialBins + k];
        }
        double frac, mean_frac, cv;
        radial_tail((double)cnt, wsum, (double)n, frac, mean_frac, cv);
        row_out[R.col_frac + tid] = frac;
        row_out[R.col_mean + tid] = mean_frac;
        row_out[R.col_cv + tid] = cv;
    }
}

int launch_roi_radial(const RadArgs& a, void* stream, uint32_t grid)
{
    if (grid == 0)
        return 0;
    const uint32_t dyn = 8u * a.m.px_cap + 4u * a.m.k_cap + 2u * a.m.step_cap;   // (<= 36 KiB: below the 64 KiB that needs an opt-in)
    hipLaunchKernelGGL(roi_radial_kernel, dim3(grid), dim3(kRB), dyn, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace nyxhip
