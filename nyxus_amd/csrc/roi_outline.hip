// roi_outline.hip -- three small shape families that need no absolute ROI position:
//   FractalDimensionFeature  FRACT_DIM_BOXCOUNT, FRACT_DIM_PERIMETER            features/fractal_dim.cpp:20-99, :127-191 (of the reference)
//   EulerNumberFeature       EULER_NUMBER (mode 8)                                features/euler_number.cpp:44-103, euler_number.h:42-69
//   RoiRadiusFeature         ROI_RADIUS_MEAN, ROI_RADIUS_MAX, ROI_RADIUS_MEDIAN   features/roi_radius.cpp:11-37
//
//   roi_outline_kernel   One 256-thread workgroup per ROI, launched like roi_radial_kernel over the contour roi_contour_kernel left in
//                        the workspace (same LDS carve: pixels | contour | step table, then the ROI's bit planes; same HBM fall-backs).
//                        Bits    the mask of the box, one bit per cell (LDS atomics; a global scratch block per workgroup when the
//                                planes exceed OutArgs::bits_cap).  The Euler number counts 2 x 2 quads 32 at a time with word logic;
//                                the box counts are popcounts -- of a pyramid of pairwise-OR'd planes (one aligned grid, padded
//                                side > 32) or of shifted row words (four grid origins, padded side <= 32).
//                        Radius  per pixel Pixel2::min_sqdist v2 over the ordered contour (contour_descent.h): integers.  Sum in
//                                64 bits, one division; the median by radix selection over ALL pixels' values.
//                        Walk    the divider walk over the contour, one stride after the other, every stride summed in a fixed
//                                tree (thread-strided partial sums, xor shuffles, four waves in order).
//                        Tail    one lane: the two least-squares slopes in fp64, the reference's operation sequence.
//   Everything that is a count is an integer, so a row depends neither on scheduling nor on the path (LDS / HBM) that served it.
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_outline.h"
#include "launch_util.h"
#include "deferred_list.h"
#include "contour_descent.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

constexpr int kOB = 256;
constexpr int kOW = kOB / 64;
constexpr int kMaxLevels = 17;                // box sizes 2 .. 65536
constexpr int kMaxStrides = 32;               // n / 4, n / 8, ..., 1 with n < 2^32

// bit i of the result = bit 2i | bit 2i + 1 of v (16 result bits)
__device__ __forceinline__ uint32_t or_pairs(uint32_t v)
{
    uint32_t t = (v | (v >> 1)) & 0x55555555u;
    t = (t | (t >> 1)) & 0x33333333u;
    t = (t | (t >> 2)) & 0x0F0F0F0Fu;
    t = (t | (t >> 4)) & 0x00FF00FFu;
    t = (t | (t >> 8)) & 0x0000FFFFu;
    return t;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// FractalDimensionFeature::loglog_slope (fractal_dim.cpp:169-191): least-squares slope of log(y) over log(x)
__device__ double loglog_slope(const double* x, const double* y, int n)
{
    double sx = 0, sy = 0, sxy = 0, sx2 = 0;
    int used = 0;
    for (int i = 0; i < n; i++) {
        if (x[i] <= 0. || y[i] <= 0.)
            continue;
        const double lx = log(x[i]), ly = log(y[i]);
        sx += lx; sy += ly; sxy += lx * ly; sx2 += lx * lx;
        used++;
    }
    if (used < 2)
        return 0.;
    const double denom = sx2 * (double)used - sx * sx;
    if (denom == 0.)
        return 0.;
    return (sxy * (double)used - sx * sy) / denom;
}

// The bit planes of one ROI in `bits` (LDS or global: the caller passes the array itself so that the accesses keep their address
// space).  Leaves the quad counts C1, C3, Cd in s_quad and the box counts in s_box[level][origin].  sweep(f): f(x, y) per pixel.
template <typename Sweep>
__device__ __forceinline__ void bit_phase(uint32_t* bits, uint32_t w, uint32_t h, uint32_t n, bool do_fr, bool do_eu, int tid, Sweep&& sweep,
                                          int* s_quad, uint32_t (*s_box)[4])
{
    const int lane = tid & 63;
    const uint32_t wd0 = w / 32u + 1u, words0 = wd0 * h;
    for (uint32_t i = (uint32_t)tid; i < words0; i += kOB) bits[i] = 0u;
    __syncthreads();
    sweep([&](uint32_t x, uint32_t y) {
        if (x < w && y < h) atomicOr(&bits[y * wd0 + (x >> 5)], 1u << (x & 31u));
    });
    __syncthreads();
    if (do_eu) {
        // quads of the padded plane (euler_number.cpp:60-97): padded row r = box row r - 1, padded column c = box column c - 1.  A task is
        // one word of a row pair; bit u of it stands for the quad whose right column is box column u (u = 0 .. w: the word behind the
        // last column exists), its left column comes in by a shift with the carry of the word before.
        uint32_t c1 = 0, c3 = 0, cd = 0;
        const uint32_t tasks = (h + 1u) * wd0;
        for (uint32_t t = (uint32_t)tid; t < tasks; t += kOB) {
            const uint32_t rb = t / wd0, j = t - rb * wd0;               // rows rb - 1 (above) and rb (below)
            uint32_t a = 0, ac = 0, b = 0, bc = 0;
            if (rb > 0) { a = bits[(rb - 1u) * wd0 + j]; if (j) ac = bits[(rb - 1u) * wd0 + j - 1u] >> 31; }
            if (rb < h) { b = bits[rb * wd0 + j]; if (j) bc = bits[rb * wd0 + j - 1u] >> 31; }
            const uint32_t q3 = (a << 1) | ac, q2 = a, q1 = (b << 1) | bc, q0 = b;   // Px bit order: 8 4 / 2 1
            const uint32_t s0 = q3 ^ q2, k0 = q3 & q2, s1 = q1 ^ q0, k1 = q1 & q0;
            c1 += (uint32_t)__popc((s0 ^ s1) & ~k0 & ~k1);                              // exactly one of four
            c3 += (uint32_t)__popc((s0 ^ s1) & (k0 | k1));                              // exactly three
            cd += (uint32_t)__popc((q3 & q0 & ~q2 & ~q1) | (q2 & q1 & ~q3 & ~q0));      // the two diagonals
        }
        c1 = wave_sum_u32(c1); c3 = wave_sum_u32(c3); cd = wave_sum_u32(cd);
        if (lane == 0) { atomicAdd(&s_quad[0], (int)c1); atomicAdd(&s_quad[1], (int)c3); atomicAdd(&s_quad[2], (int)cd); }
    }
    if (do_fr && n >= 2) {
        const uint32_t P = outline_ceil_pow2(w > h ? w : h);
        const int L = 31 - __clz((int)P);                                  // box sizes 2^1 .. 2^L
        if (P > 32u) {
            // one aligned grid per box size (fractal_dim.cpp:45-59): level k = level k - 1 with 2 x 2 cells OR'd together
            const uint32_t* src = bits;
            uint32_t* dst = bits + words0;
            uint32_t swd = wd0, srows = h;
            for (int k = 1; k <= L; k++) {
                const uint32_t dwd = (swd + 1u) / 2u, drows = (srows + 1u) / 2u, tasks = dwd * drows;
                uint32_t cnt = 0;
                for (uint32_t t = (uint32_t)tid; t < tasks; t += kOB) {
                    const uint32_t r = t / dwd, j = t - r * dwd;
                    const uint32_t* r0 = src + (2u * r) * swd + 2u * j;
                    const bool two_w = 2u * j + 1u < swd, two_r = 2u * r + 1u < srows;
                    uint32_t lo = r0[0], hi = two_w ? r0[1] : 0u;
                    if (two_r) { lo |= r0[swd]; if (two_w) hi |= r0[swd + 1u]; }
                    const uint32_t o = or_pairs(lo) | (or_pairs(hi) << 16);
                    dst[t] = o;
                    cnt += (uint32_t)__popc(o);
                }
                cnt = wave_sum_u32(cnt);
                if (lane == 0 && cnt) atomicAdd(&s_box[k][0], cnt);
                __syncthreads();
                src = dst; dst += tasks; swd = dwd; srows = drows;
            }
        } else {
            // shifting grids (fractal_dim.cpp:61-96): box size s = 2^k, origins {0, s / 2}^2, span = P / s + 2 boxes per axis.  A task is
            // one row of boxes of one (size, origin): the OR of its box rows, shifted by the origin, cut into groups of s bits.
            const uint32_t tasks = (uint32_t)L * 4u * 18u;
            for (uint32_t t = (uint32_t)tid; t < tasks; t += kOB) {
                const int k = (int)(t / 72u) + 1;
                const uint32_t o = (t % 72u) / 18u, br = t % 18u, s = 1u << k, span = (P >> k) + 2u;
                if (br >= span) continue;
                const uint32_t ox = (o & 1u) * s / 2u, oy = (o >> 1) * s / 2u;
                const int y0 = (int)(br * s) - (int)oy;
                uint32_t wd = 0;
                for (int yy = y0 < 0 ? 0 : y0; yy < y0 + (int)s && yy < (int)h; yy++) wd |= bits[(uint32_t)yy * wd0];
                if (!wd) continue;
                const unsigned long long v = (unsigned long long)wd << ox, m = (1ull << s) - 1ull;
                uint32_t cnt = 0;
                for (uint32_t c = 0; c < span && c * s < 64u; c++) cnt += ((v >> (c * s)) & m) != 0ull;
                atomicAdd(&s_box[k][o], cnt);
            }
        }
    }
    __syncthreads();
}

} // namespace

__global__ __launch_bounds__(kOB) void roi_outline_kernel(const OutArgs R)
{
    const MomArgs& A = R.m;
    __shared__ unsigned long long s_sum[kOW];
    __shared__ uint32_t s_max[kOW];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_sel[4];                                         // bin, count before it, count in it | smallest value above the left median
    __shared__ int s_quad[3];                                             // C1, C3, Cd
    __shared__ uint32_t s_box[kMaxLevels][4];                             // box counts per size and grid origin
    __shared__ double s_walk[kMaxStrides][kOW];                           // divider walk: per stride the four waves' partial sums
    __shared__ double s_pt[2][kMaxStrides];                               // the points of a least-squares fit (one lane; indexed: not registers)
    // staged pixels | contour | step table: the carve of the moments kernel; the bit planes behind it
    extern __shared__ __attribute__((aligned(16))) unsigned char out_lds[];
    uint2* const s_px = (uint2*)out_lds;                                  // [A.px_cap]  x | y << 16, squared distance to the contour
    uint32_t* const s_K = (uint32_t*)(out_lds + 8u * A.px_cap);           // [A.k_cap]
    uint16_t* const s_step = (uint16_t*)(s_K + A.k_cap);                  // [A.step_cap]
    uint32_t* const s_bits = (uint32_t*)(out_lds + 8u * A.px_cap + 4u * A.k_cap + ((2u * A.step_cap + 15u) & ~15u));   // [R.bits_cap]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t roi = A.sp.roi_index ? A.sp.roi_index[blockIdx.x] : blockIdx.x;   // (a list: the big boxes of a batch)
    if (roi >= A.n_roi)
        return;
    const bool do_fr = (R.fams & NYXHIP_FAM_FRACTAL) != 0, do_eu = (R.fams & NYXHIP_FAM_EULER) != 0, do_rr = (R.fams & NYXHIP_FAM_ROI_RADIUS) != 0;
    const uint64_t off = A.px_offset[roi];
    const uint32_t n = (uint32_t)(A.px_offset[roi + 1] - off);
    const uint32_t bw_ = A.bbox_w[roi], bh_ = A.bbox_h[roi];
    if (R.has_contour && A.sp.defer_large && (uint64_t)(bw_ + 2u) * (bh_ + 2u) > A.plane_cap)
        return;                                                           // served by the launch over the big-box list
    double* const row_out = A.out + roi * A.ld;
    auto write_row = [&](double box, double per, double eul, double mean, double mx, double med) {
        if (tid != 0) return;
        if (do_fr) { row_out[R.col_fractal] = box; row_out[R.col_fractal + 1] = per; }
        if (do_eu) row_out[R.col_euler] = eul;
        if (do_rr) { row_out[R.col_radius] = mean; row_out[R.col_radius + 1] = mx; row_out[R.col_radius + 2] = med; }
    };
    const uint64_t words = (do_fr || do_eu) ? outline_bit_words(bw_, bh_, do_fr) : 0ull;
    const bool bits_lds = words <= R.bits_cap;
    if (!bits_lds) {
        if (R.defer_bits)
            return;                                                       // served by the launch over the list of such ROIs
        if (!R.bits_ws || words > R.bits_stride) {                        // (a box beyond what the caller stated)
            if (tid == 0) atomicCAS(A.status, 0, NYXHIP_ERR_ROI_TOO_LARGE);
            const double qnan = __longlong_as_double(0x7ff8000000000000LL);
            write_row(qnan, qnan, qnan, qnan, qnan, qnan);
            return;
        }
    }
    if (n == 0) { write_row(0.0, 0.0, 0.0, 0.0, 0.0, 0.0); return; }
    const int nK = R.has_contour ? (int)A.n_contour[roi] : 0;
    const bool small_xy = bw_ + 2u < 32768u && bh_ + 2u < 32768u;         // integer distances are exact (sqdist_descent)
    const uint32_t* K = A.ws_contour + off;
    const bool k_lds = nK <= (int)A.k_cap;
    if (k_lds && nK > 0) {
        for (int i = tid; i < nK; i += kOB) s_K[i] = K[i];
        K = s_K;
    }
    // window width -> step of the hill descent (first step from n, later ones from windows of at most two steps)
    const int step0 = __builtin_amdgcn_readfirstlane(nK >= 2 ? (int)((double)nK / log((double)nK)) : 1);
    const int tab_n = min((int)A.step_cap, 2 * step0 + 2);
    if (do_rr && nK > 0)
        for (int m = 11 + tid; m < tab_n; m += kOB) s_step[m] = (uint16_t)(int)((double)m / log((double)m));
    const bool staged = n <= A.px_cap;
    if (staged)
        for_each_cloud_pixel<kOB>(A.inten + off, A.x + off, A.y + off, n, tid, [&](uint32_t i, uint32_t, uint32_t xi, uint32_t yi) {
            s_px[i] = make_uint2(xi | (yi << 16), 0u);
        });
    if (tid < 3) s_quad[tid] = 0;
    if (tid < kMaxLevels * 4) (&s_box[0][0])[tid] = 0u;
    if (tid == 0) s_sel[3] = 0xFFFFFFFFu;
    __syncthreads();
    auto sweep = [&](auto&& body) {                      // body(i, x, y) for this thread's pixels i = tid, tid + 256, ...
        if (staged) {
            for (uint32_t i = (uint32_t)tid; i < n; i += kOB) {
                const uint32_t q = s_px[i].x;
                body(i, q & 0xFFFFu, q >> 16);
            }
        } else
            for_each_cloud_pixel<kOB>(A.inten + off, A.x + off, A.y + off, n, tid, [&](uint32_t i, uint32_t, uint32_t xi, uint32_t yi) { body(i, xi, yi); });
    };
    // ---- bit planes: Euler number and box counts ----------------------------------------------------------------------------
    if (do_fr || do_eu) {
        auto sweep_xy = [&](auto&& f) { sweep([&](uint32_t, uint32_t x, uint32_t y) { f(x, y); }); };
        if (bits_lds) bit_phase(s_bits, bw_, bh_, n, do_fr, do_eu, tid, sweep_xy, s_quad, s_box);
        else bit_phase(R.bits_ws + (uint64_t)blockIdx.x * R.bits_stride, bw_, bh_, n, do_fr, do_eu, tid, sweep_xy, s_quad, s_box);
    }
    // ---- ROI radius (roi_radius.cpp:11-37) -----------------------------------------------------------------------------------
    double r_mean = 0.0, r_max = 0.0, r_med = 0.0;
    if (do_rr && nK > 0) {
        // the values of an ROI beyond the LDS carve go to the ROI's own span of the per-pixel workspace plane, which every earlier
        // reader of this stream is done with (8 bytes per pixel there, 4 used)
        uint32_t* const d_ws = (uint32_t*)(A.ws_L + off);
        unsigned long long sum = 0;
        uint32_t mx = 0;
        sweep([&](uint32_t i, uint32_t xi, uint32_t yi) {
            double d;
            if (!small_xy) d = min_sqdist_v2<false>((int)xi, (int)yi, K, nK, step0, s_step, tab_n);
            else if (k_lds) d = min_sqdist_v2<true>((int)xi, (int)yi, s_K, nK, step0, s_step, tab_n);
            else d = min_sqdist_v2<true>((int)xi, (int)yi, K, nK, step0, s_step, tab_n);
            const uint32_t du = d < 4294967295.0 ? (uint32_t)d : 0xFFFFFFFFu;   // HistoItem is unsigned (boxes beyond 46340 a side could exceed it)
            if (staged) s_px[i].y = du; else d_ws[i] = du;
            sum += du;
            mx = du > mx ? du : mx;
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, 64);
            const uint32_t om = __shfl_xor(mx, o, 64);
            mx = om > mx ? om : mx;
        }
        if (lane == 0) { s_sum[wave] = sum; s_max[wave] = mx; }
        __syncthreads();                                                  // (also: every value is stored)
        sum = 0; mx = 0;
#pragma unroll
        for (int w = 0; w < kOW; w++) { sum += s_sum[w]; mx = s_max[w] > mx ? s_max[w] : mx; }
        r_mean = (double)sum / (double)n;
        r_max = (double)mx;
        // median (histogram.h:268-287 over ALL values): radix selection of rank n / 2 (odd) or n / 2 - 1 (even), a byte per pass,
        // from the highest byte the maximum has
        auto val = [&](uint32_t i) -> uint32_t { return staged ? s_px[i].y : d_ws[i]; };
        uint32_t rank = (n & 1u) ? n / 2u : n / 2u - 1u, prefix = 0, in_bin = 0;
        const int top = mx >> 24 ? 24 : mx >> 16 ? 16 : mx >> 8 ? 8 : 0;
        for (int sh = top; sh >= 0; sh -= 8) {
            s_hist[tid] = 0u;
            __syncthreads();
            for (uint32_t i = (uint32_t)tid; i < n; i += kOB) {
                const uint32_t v = val(i);
                if (sh == 24 || (v >> (sh + 8)) == prefix) atomicAdd(&s_hist[(v >> sh) & 255u], 1u);
            }
            __syncthreads();
            if (wave == 0) {
                const uint32_t c0 = s_hist[4 * lane], c1 = s_hist[4 * lane + 1], c2 = s_hist[4 * lane + 2], c3 = s_hist[4 * lane + 3];
                uint32_t incl = c0 + c1 + c2 + c3;
                const uint32_t tot = incl;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t up = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += up;
                }
                uint32_t before = incl - tot;
                if (rank >= before && rank < incl) {                      // exactly one lane
                    uint32_t bin = 4u * lane, c = c0;
                    if (rank >= before + c) { before += c; bin++; c = c1;
                        if (rank >= before + c) { before += c; bin++; c = c2;
                            if (rank >= before + c) { before += c; bin++; c = c3; } } }
                    s_sel[0] = bin; s_sel[1] = before; s_sel[2] = c;
                }
            }
            __syncthreads();
            prefix = (prefix << 8) | s_sel[0];
            rank -= s_sel[1];
            in_bin = s_sel[2];
        }
        const uint32_t left = prefix;
        if (n & 1u)
            r_med = (double)left;
        else {
            uint32_t right = left;
            if (rank + 1u >= in_bin) {                                    // the next rank lies above the run of `left`
                uint32_t mn = 0xFFFFFFFFu;
                for (uint32_t i = (uint32_t)tid; i < n; i += kOB) {
                    const uint32_t v = val(i);
                    if (v > left && v < mn) mn = v;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const uint32_t om = __shfl_xor(mn, o, 64);
                    mn = om < mn ? om : mn;
                }
                if (lane == 0) atomicMin(&s_sel[3], mn);
                __syncthreads();
                right = s_sel[3];
            }
            r_med = (double)(uint32_t)(right + left) / 2.0;               // double(right + left) / 2.0 on unsigned operands
        }
    }
    // ---- divider walk over the closed contour (fractal_dim.cpp:127-167) --------------------------------------------------------
    int n_strides = 0;
    if (do_fr && nK >= 3) {
        for (uint32_t s = (uint32_t)nK / 4u; s > 0; s /= 2u, n_strides++) {
            const uint32_t m = ((uint32_t)nK - 1u) / s;                   // chords 0 .. m - 1 forward, chord m closes the loop
            double part = 0.0;
            for (uint32_t j = (uint32_t)tid; j <= m; j += kOB) {
                const uint32_t p = K[j * s], q = K[j < m ? (j + 1u) * s : 0u];
                const long long dx = (long long)(p & 0xFFFFu) - (long long)(q & 0xFFFFu), dy = (long long)(p >> 16) - (long long)(q >> 16);
                part += sqrt((double)(dx * dx + dy * dy));
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
            if (lane == 0) s_walk[n_strides][wave] = part;
        }
        __syncthreads();
    }
    // ---- tail ------------------------------------------------------------------------------------------------------------------
    if (tid == 0) {
        double box_fd = 0.0, per_fd = 0.0, eul = 0.0;
        if (do_eu) {
            const long c1 = s_quad[0], c3 = s_quad[1], cd = s_quad[2];
            eul = (double)((c1 - c3 - 2 * cd) / 4);                       // euler_number.cpp:102 (integer division)
        }
        if (do_fr) {
            double* const x = s_pt[0];
            double* const y = s_pt[1];
            if (n >= 2) {
                const uint32_t P = outline_ceil_pow2(bw_ > bh_ ? bw_ : bh_);
                const int L = 31 - __clz((int)P);
                int np = 0;
                for (int k = L; k >= 1; k--, np++) {
                    uint32_t c = s_box[k][0];
                    if (P <= 32u)
                        for (int o = 1; o < 4; o++) c = s_box[k][o] < c ? s_box[k][o] : c;
                    x[np] = (double)(1u << k); y[np] = (double)c;
                }
                box_fd = -loglog_slope(x, y, np);
            }
            if (nK >= 3) {
                int i = 0;
                for (uint32_t s = (uint32_t)nK / 4u; s > 0; s /= 2u, i++) {
                    const double perim = (s_walk[i][0] + s_walk[i][1]) + (s_walk[i][2] + s_walk[i][3]);
                    const double nsteps = (double)(((uint32_t)nK - 1u) / s + 1u);
                    x[i] = perim / nsteps; y[i] = perim;
                }
                per_fd = 1.0 - loglog_slope(x, y, i);
            }
        }
        write_row(box_fd, per_fd, eul, r_mean, r_max, r_med);
    }
}

__device__ bool OutlineBitsBig::operator()(uint64_t i, uint32_t*) const
{
    return outline_bit_words(bw[i], bh[i], pyramid != 0) > cap;
}
template int deferred_classify<OutlineBitsBig>(uint64_t, const OutlineBitsBig&, uint32_t*, hipStream_t);

int launch_roi_outline(const OutArgs& a, void* stream, uint32_t grid)
{
    if (grid == 0)
        return 0;
    // (<= 24 + 8 + 4 + 8 KiB: below the 64 KiB that needs an opt-in)
    const uint32_t dyn = 8u * a.m.px_cap + 4u * a.m.k_cap + ((2u * a.m.step_cap + 15u) & ~15u) + 4u * a.bits_cap;
    hipLaunchKernelGGL(roi_outline_kernel, dim3(grid), dim3(kOB), dyn, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace nyxhip
