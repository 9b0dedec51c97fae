// roi_erosion.hip -- two classes of the shape block that read the pixel cloud only (no contour, no staged pixels):
//   ErosionPixelsFeature   (features/erosion.cpp:20-109 of the reference, and the aux_min == aux_max skip of :147-164)
//   EllipseFittingFeature  (features/ellipse_fitting.cpp:26-82; centroid and area: basic_morphology.cpp:21-47)
//
//   roi_erosion_kernel   One 256-thread workgroup per ROI.  The mask of the w x h box is a bit plane, rows of w / 32 + 1 words (the
//                        layout of roi_outline.hip), set by atomic OR whatever the intensity.  A pass gives one lane one word at a
//                        time: the word AND its two shifted forms (with the carry bits of the neighbouring words) AND the rows above
//                        and below, taken under the interior mask -- columns 2 <= c < w - 1, rows 2 <= r < h - 1, the asymmetric
//                        range of the reference's loops; every other cell is copied.  Two planes, ping-pong; the updated cells that
//                        are still set are counted (popcount) and summed over the workgroup.  Count 0 at pass k: the value is k.
//                        A pass can only clear cells, so a pass that changes no word while its count is non-zero has reached a fixed
//                        point: every later pass is the same, the reference runs into SANITY_MAX_NUM_EROSIONS, the value is 1000 at
//                        once.  One barrier per pass (three rotating counter slots).
//                        ROIs whose two planes exceed the LDS planes are served by a launch over their list with the planes in
//                        global memory (EroArgs::ws); the code is the same.  The value is an integer: every path gives the same bits.
//   roi_ellipse_wave_kernel / roi_ellipse_block_kernel
//                        n, sum x, sum y, sum x^2, sum y^2, sum xy of the box-relative coordinates in u64 (coordinates are 16 bits, so
//                        no sum can overflow for any box the ABI can state), a wave per ROI of <= kEllipseWavePx pixels and a
//                        workgroup per larger ROI.  One lane closes: the central second moments' numerators n * Sxx - Sx^2, ... are
//                        formed exactly in 128 bits, rounded to fp64 once, and the six columns follow with the reference's
//                        expressions.  Integer sums: the row depends neither on scheduling nor on which kernel served the ROI.
//   Built with -ffp-contract=off like every unit; no reciprocal forms.
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_erosion.h"
#include "launch_util.h"
#include "deferred_list.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

constexpr int kEB = 256;
constexpr int kEW = kEB / 64;

__device__ __forceinline__ uint32_t ero_sum_u32(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                                                                // (lane 0 holds the sum)
}
__device__ __forceinline__ unsigned long long ero_sum_u64(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// bits of word j of a row that the reference's loops update: columns 2 <= c < w - 1
__device__ __forceinline__ uint32_t erosion_col_mask(uint32_t j, uint32_t w)
{
    const uint32_t c0 = 32u * j;
    const uint32_t lo = c0 >= 2u ? 0u : 2u - c0;                             // first updated bit of the word
    if (w < 4u || c0 + lo >= w - 1u) return 0u;
    const uint32_t hi = (w - 1u - c0) >= 32u ? 32u : (w - 1u - c0);          // one behind the last updated bit
    const uint32_t upto = hi >= 32u ? 0xFFFFFFFFu : ((1u << hi) - 1u);
    return upto & ~((1u << lo) - 1u);
}

struct EroShared {
    uint32_t cnt[3];
    uint32_t chg[3];
};

// The erosion chain of one ROI on two planes of `words` words each at `A` and `B`.  Returns the value on every thread.
template <bool kGlobal>
__device__ uint32_t erosion_body(EroShared& S, uint32_t* A, uint32_t* B, uint32_t words, const uint16_t* x, const uint16_t* y, uint32_t n, uint32_t w,
                                 uint32_t h, int tid)
{
    const uint32_t wpr = w / 32u + 1u;
    for (uint32_t i = tid; i < words; i += kEB) A[i] = 0u;
    if (tid < 3) { S.cnt[tid] = 0u; S.chg[tid] = 0u; }
    blk_sync<kGlobal>();
    for (uint32_t i = tid; i < n; i += kEB) {
        const uint32_t px = x[i], py = y[i];
        if (px < w && py < h)                                                // (a pixel outside its stated box is not in the mask)
            atomicOr(&A[py * wpr + (px >> 5)], 1u << (px & 31u));
    }
    blk_sync<kGlobal>();
    if (w < 4u || h < 4u)
        return 0u;                                                           // both loops are empty: numNon0 == 0 at k == 0
    uint32_t value = (uint32_t)kErosionMaxPasses;
    for (uint32_t k = 0; k < (uint32_t)kErosionMaxPasses; k++) {
        const uint32_t slot = k % 3u;
        if (tid == 0) { S.cnt[(k + 1u) % 3u] = 0u; S.chg[(k + 1u) % 3u] = 0u; }
        uint32_t cnt = 0u, chg = 0u;
        for (uint32_t i = tid; i < words; i += kEB) {
            const uint32_t r = i / wpr, j = i - r * wpr;
            const uint32_t cur = A[i];
            uint32_t nw = cur;
            if (r >= 2u && r + 1u < h) {
                const uint32_t m = erosion_col_mask(j, w);
                if (m) {
                    const uint32_t lf = (cur << 1) | (j > 0u ? A[i - 1u] >> 31 : 0u);          // bit c: cell c - 1
                    const uint32_t rt = (cur >> 1) | (j + 1u < wpr ? A[i + 1u] << 31 : 0u);    // bit c: cell c + 1
                    const uint32_t er = cur & lf & rt & A[i - wpr] & A[i + wpr];
                    nw = (cur & ~m) | (er & m);
                    cnt += (uint32_t)__popc(er & m);
                }
            }
            B[i] = nw;
            chg |= nw ^ cur;
        }
        cnt = ero_sum_u32(cnt);
        const unsigned long long any = __ballot(chg != 0u);
        if ((tid & 63) == 0) {
            if (cnt) atomicAdd(&S.cnt[slot], cnt);
            if (any) atomicOr(&S.chg[slot], 1u);
        }
        blk_sync<kGlobal>();
        const uint32_t total = S.cnt[slot], changed = S.chg[slot];
        if (total == 0u) { value = k; break; }
        if (changed == 0u) break;                                            // a fixed point that is not empty: 1000
        uint32_t* t = A; A = B; B = t;
    }
    return value;
}

__host__ __device__ inline bool erosion_listed(uint32_t w, uint32_t h, uint32_t lds_words)
{
    return 2ull * erosion_plane_words(w, h) > (uint64_t)lds_words;
}

// ---- ellipse ----------------------------------------------------------------------------------------------------------------

struct U128 { unsigned long long hi, lo; };

__device__ __forceinline__ U128 mul_u64(unsigned long long a, unsigned long long b)
{
    U128 r;
    r.lo = a * b;
    r.hi = __umul64hi(a, b);
    return r;
}
// a - b for a >= b
__device__ __forceinline__ U128 sub_u128(U128 a, U128 b)
{
    U128 r;
    r.lo = a.lo - b.lo;
    r.hi = a.hi - b.hi - (a.lo < b.lo ? 1ull : 0ull);
    return r;
}
__device__ __forceinline__ bool less_u128(U128 a, U128 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ double to_double(U128 a) { return (double)a.hi * 18446744073709551616.0 + (double)a.lo; }

struct EllSums { unsigned long long sx, sy, sxx, syy, sxy; };

__device__ __forceinline__ void ell_add(EllSums& s, uint32_t px, uint32_t py)
{
    s.sx += px; s.sy += py;
    s.sxx += (unsigned long long)(px * px); s.syy += (unsigned long long)(py * py); s.sxy += (unsigned long long)(px * py);   // (16-bit factors)
}

// The six columns from the sums (one lane): ellipse_fitting.cpp:48-81 on uxx, uyy, uxy formed from exact integers.
__device__ void ellipse_close(unsigned long long n, const EllSums& s, double* o)
{
    const U128 nxx = sub_u128(mul_u64(n, s.sxx), mul_u64(s.sx, s.sx));       // n * Sxx - Sx^2 >= 0 (Cauchy-Schwarz)
    const U128 nyy = sub_u128(mul_u64(n, s.syy), mul_u64(s.sy, s.sy));
    const U128 pa = mul_u64(n, s.sxy), pb = mul_u64(s.sx, s.sy);
    const bool neg = less_u128(pa, pb);
    const U128 nxy = neg ? sub_u128(pb, pa) : sub_u128(pa, pb);
    const bool uxy_zero = (nxy.hi | nxy.lo) == 0ull;                         // the exact identity n * Sxy == Sx * Sy
    const double nn = (double)n * (double)n;
    const double uxx = to_double(nxx) / nn + 1. / 12.;
    const double uyy = to_double(nyy) / nn + 1. / 12.;
    double uxy = to_double(nxy) / nn;
    if (neg) uxy = -uxy;
    const double common = sqrt((uxx - uyy) * (uxx - uyy) + 4. * uxy * uxy);
    const double major = 2. * sqrt(2.) * sqrt(uxx + uyy + common);
    const double minor = 2. * sqrt(2.) * sqrt(uxx + uyy - common);
    const double ecc = sqrt(1.0 - minor * minor / (major * major));
    const double elong = minor / major;
    const double round_ = (4. * (double)n) / (3.14159265358979323846 * major * major);
    double num, den;
    if (uyy > uxx) {
        num = uyy - uxx + sqrt((uyy - uxx) * (uyy - uxx) + 4 * uxy * uxy);
        den = 2 * uxy;
    } else {
        num = 2 * uxy;
        den = uxx - uyy + sqrt((uxx - uyy) * (uxx - uyy) + 4 * uxy * uxy);
    }
    double orient;
    if (uxy_zero)
        orient = uxx >= uyy ? 0. : 90.;
    else
        orient = 180. / 3.14159265358979323846 * atan(num / den);
    o[0] = major; o[1] = minor; o[2] = elong; o[3] = ecc; o[4] = orient; o[5] = round_;
}

} // namespace

__global__ __launch_bounds__(kEB) void roi_erosion_kernel(const EroArgs R)
{
    __shared__ EroShared S;
    extern __shared__ __attribute__((aligned(16))) uint32_t erosion_lds[];   // [R.lds_words]
    const int tid = threadIdx.x;
    const uint64_t roi = R.roi_index ? R.roi_index[blockIdx.x] : blockIdx.x;
    if (roi >= R.n_roi)
        return;
    const uint32_t w = R.bbox_w[roi], h = R.bbox_h[roi];
    const bool listed = erosion_listed(w, h, R.lds_words);
    if (R.roi_index ? !listed : (listed && R.defer_large))
        return;                                                              // served by the other launch
    const uint64_t off = R.px_offset[roi];
    const uint64_t n64 = R.px_offset[roi + 1] - off;
    double* const o = R.out + roi * R.ld + R.col_erosion;
    if (listed && !R.roi_index) {                                            // the batch's stated extrema did not cover this box
        if (tid == 0) {
            atomicCAS(R.status, 0, NYXHIP_ERR_ROI_TOO_LARGE);
            o[0] = o[1] = __longlong_as_double(0x7ff8000000000000LL);
        }
        return;
    }
    if (tid == 0) o[1] = 0.0;                                                // EROSIONS_2_VANISH_COMPLEMENT: the class never assigns it
    if (n64 == 0 || R.min_inten[roi] == R.max_inten[roi]) {                  // the driver's skip (erosion.cpp:157-158): the initial 0
        if (tid == 0) o[0] = 0.0;
        return;
    }
    const uint64_t words = erosion_plane_words(w, h);
    if (n64 > 0xFFFFFFFFull || words > 0x7FFFFFFFull || (listed && (!R.ws || 2ull * words > R.ws_stride))) {
        if (tid == 0) {
            atomicCAS(R.status, 0, NYXHIP_ERR_ROI_TOO_LARGE);
            o[0] = __longlong_as_double(0x7ff8000000000000LL);
        }
        return;
    }
    uint32_t v;
    if (listed) {
        uint32_t* const ws = R.ws + (uint64_t)blockIdx.x * R.ws_stride;
        v = erosion_body<true>(S, ws, ws + words, (uint32_t)words, R.x + off, R.y + off, (uint32_t)n64, w, h, tid);
    } else {
        v = erosion_body<false>(S, erosion_lds, erosion_lds + words, (uint32_t)words, R.x + off, R.y + off, (uint32_t)n64, w, h, tid);
    }
    if (tid == 0) o[0] = (double)v;
}

__device__ bool ErosionListed::operator()(uint64_t i, uint32_t* hdr) const
{
    if (!erosion_listed(bw[i], bh[i], cap)) return false;
    const uint64_t pw = erosion_plane_words(bw[i], bh[i]);
    atomicMax(&hdr[1], pw > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)pw);
    return true;
}
template int deferred_classify<ErosionListed>(uint64_t, const ErosionListed&, uint32_t*, hipStream_t);

// a wave per ROI: workgroup b, wave v serves ROI kEW * b + v when it has at most kEllipseWavePx pixels
__global__ __launch_bounds__(kEB) void roi_ellipse_wave_kernel(const EroArgs R)
{
    const int lane = threadIdx.x & 63;
    const uint64_t roi = (uint64_t)blockIdx.x * kEW + (threadIdx.x >> 6);
    if (roi >= R.n_roi)
        return;
    const uint64_t off = R.px_offset[roi];
    const uint64_t n = R.px_offset[roi + 1] - off;
    if (n > kEllipseWavePx)
        return;                                                              // the workgroup kernel's
    double* const o = R.out + roi * R.ld + R.col_ellipse;
    if (n == 0) {
        if (lane < kEllipseCols) o[lane] = 0.0;
        return;
    }
    EllSums s = {0, 0, 0, 0, 0};
    for (uint32_t i = lane; i < (uint32_t)n; i += 64)
        ell_add(s, R.x[off + i], R.y[off + i]);
    s.sx = ero_sum_u64(s.sx); s.sy = ero_sum_u64(s.sy);
    s.sxx = ero_sum_u64(s.sxx); s.syy = ero_sum_u64(s.syy); s.sxy = ero_sum_u64(s.sxy);
    if (lane == 0)
        ellipse_close(n, s, o);
}

// a workgroup per ROI of more than kEllipseWavePx pixels
__global__ __launch_bounds__(kEB) void roi_ellipse_block_kernel(const EroArgs R)
{
    __shared__ unsigned long long red[kEW][5];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t roi = blockIdx.x;
    if (roi >= R.n_roi)
        return;
    const uint64_t off = R.px_offset[roi];
    const uint64_t n = R.px_offset[roi + 1] - off;
    if (n <= kEllipseWavePx)
        return;                                                              // the wave kernel's
    EllSums s = {0, 0, 0, 0, 0};
    for (uint64_t i = tid; i < n; i += kEB)
        ell_add(s, R.x[off + i], R.y[off + i]);
    s.sx = ero_sum_u64(s.sx); s.sy = ero_sum_u64(s.sy);
    s.sxx = ero_sum_u64(s.sxx); s.syy = ero_sum_u64(s.syy); s.sxy = ero_sum_u64(s.sxy);
    if (lane == 0) { red[wv][0] = s.sx; red[wv][1] = s.sy; red[wv][2] = s.sxx; red[wv][3] = s.syy; red[wv][4] = s.sxy; }
    __syncthreads();
    if (tid == 0) {
        EllSums t = {0, 0, 0, 0, 0};
        for (int k = 0; k < kEW; k++) { t.sx += red[k][0]; t.sy += red[k][1]; t.sxx += red[k][2]; t.syy += red[k][3]; t.sxy += red[k][4]; }
        ellipse_close(n, t, R.out + roi * R.ld + R.col_ellipse);
    }
}

int launch_roi_erosion(const EroArgs& a, void* stream, uint32_t grid)
{
    if (grid == 0)
        return 0;
    const uint32_t dyn = 4u * (a.roi_index ? 0u : a.lds_words);              // (<= 32 KiB)
    hipLaunchKernelGGL(roi_erosion_kernel, dim3(grid), dim3(kEB), dyn, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_roi_ellipse(const EroArgs& a, void* stream, bool with_large)
{
    if (a.n_roi == 0)
        return 0;
    hipLaunchKernelGGL(roi_ellipse_wave_kernel, dim3((unsigned)((a.n_roi + kEW - 1) / kEW)), dim3(kEB), 0, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess)
        return 1;
    if (with_large) {
        hipLaunchKernelGGL(roi_ellipse_block_kernel, dim3((unsigned)a.n_roi), dim3(kEB), 0, (hipStream_t)stream, a);
        if (hipGetLastError() != hipSuccess)
            return 1;
    }
    return 0;
}

} // namespace nyxhip
