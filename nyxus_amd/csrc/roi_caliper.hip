// roi_caliper.hip -- the three caliper classes of the shape block, on the convex hull turned in steps of 10 degrees:
//   CaliperFeretFeature        MIN_FERET_ANGLE, MAX_FERET_ANGLE, STAT_FERET_DIAM_*   features/caliper_feret.cpp:80-104 (of the reference)
//   CaliperMartinFeature       STAT_MARTIN_DIAM_*                                     features/caliper_martin.cpp:16-43, :89-137
//   CaliperNassensteinFeature  STAT_NASSENSTEIN_DIAM_*                                features/caliper_nassenstein.cpp:16-43, :89-126
// on ConvexHullFeature::build_convex_hull (convex_hull_nontriv.cpp:68-120), Rotation::rotate_around_center_fp (rotation.cpp:37-68)
// and ComputeCommonStatistics2 (common_stats.cpp:9-72).
//
//   roi_caliper_kernel   One 256-thread workgroup per ROI; needs the pixel cloud only (no contour).
//                        Columns   the lowest and the highest pixel of every box column (integer LDS atomics; a global scratch block
//                                  per workgroup when the box is wider than CalArgs::cols_cap): a hull vertex is one of them.
//                        Hull      one lane: the reference's monotone chain over those <= 2 w points in (x, y) order -- the upper
//                                  chain, then the lower chain's points that are not present yet, in the reference's vertex order.
//                        Angles    one after the other: every thread turns its vertices about the mean vertex in fp64 (sin / cos from
//                                  the host, in the kernel arguments), rounds them to float as the reference stores them; then 100
//                                  lanes cut the hull at Martin's levels while a lane of another wave measures Nassenstein's chord.
//                        Tail      18 lanes walk Martin's cumulative widths (sequential sums: the walk selects a level), then one
//                                  lane per class closes the statistics over its <= 19 diameters.
//   Everything order-sensitive is an integer or a fixed sequence of fp64 operations: a row depends neither on scheduling nor on the
//   path (LDS / HBM) nor on the pixel order.  Built with -ffp-contract=off like every unit; no reciprocal forms.
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_caliper.h"
#include "launch_util.h"
#include "deferred_list.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

constexpr int kCB = 256;
constexpr int kCW = kCB / 64;
constexpr uint32_t kNoPoint = 0xFFFFFFFFu;    // (a box is at most 65535 wide: x = 65535 does not occur)

// ConvexHullFeature::right_turn on points x | y << 16
__device__ __forceinline__ bool right_turn(uint32_t p1, uint32_t p2, uint32_t p3)
{
    const long long x1 = p1 & 0xFFFFu, y1 = p1 >> 16, x2 = p2 & 0xFFFFu, y2 = p2 >> 16, x3 = p3 & 0xFFFFu, y3 = p3 >> 16;
    return (x3 - x1) * (y2 - y1) - (y3 - y1) * (x2 - x1) > 0;
}

// hull_width_at_y (kCutY: the cut is y = v, the extent is along x) / hull_height_at_x (the cut is x = v, the extent along y)
template <bool kCutY>
__device__ __forceinline__ double span_at(const float2* P, int n, double v)
{
    bool have = false;
    double lo = 0.0, hi = 0.0;
    float2 a = P[0];
    for (int i = 0; i < n; i++) {
        const float2 b = P[i + 1 < n ? i + 1 : 0];
        const float a_c = kCutY ? a.y : a.x, b_c = kCutY ? b.y : b.x;      // along the cut's normal
        const float a_o = kCutY ? a.x : a.y, b_o = kCutY ? b.x : b.y;      // along the cut
        const double ac = a_c, bc = b_c, mn = bc < ac ? bc : ac, mx = ac < bc ? bc : ac;
        a = b;
        if (v < mn || v > mx)
            continue;
        double e0, e1;
        if (bc != ac) {
            const float d = b_o - a_o;                                      // (float operands: a float difference, as in the reference)
            e0 = e1 = (double)a_o + (double)d * (v - ac) / (bc - ac);
        } else {
            const double ao = a_o, bo = b_o;
            e0 = bo < ao ? bo : ao;
            e1 = ao < bo ? bo : ao;
        }
        if (!have) { lo = e0; hi = e1; have = true; }
        else { lo = e0 < lo ? e0 : lo; hi = hi < e1 ? e1 : hi; }
    }
    return have ? hi - lo : 0.0;
}

// ComputeCommonStatistics2 over D[0 .. n) (LDS; sorted on return): min, max, mean, median, stddev, mode -> o[0 .. 6)
__device__ void common_stats(double* D, int n, double* o)
{
    if (n == 0) {
        for (int i = 0; i < 6; i++) o[i] = 0.0;
        return;
    }
    double mx = D[0], mn = D[0], sum = 0.0;
    for (int i = 0; i < n; i++) {
        mx = mx < D[i] ? D[i] : mx;
        mn = D[i] < mn ? D[i] : mn;
        sum += D[i];
    }
    const double mean = sum / (double)n;
    double ss = 0.0;
    for (int i = 0; i < n; i++) ss += (D[i] - mean) * (D[i] - mean);
    const double sd = sqrt(ss / (double)n);
    // the first bin of the truncation histogram that holds the largest count
    const int int_min = (int)floor(mn);
    int best = 0, best_bin = -1;
    for (int i = 0; i < n; i++) {
        const int bi = (int)D[i] - int_min;
        int c = 0;
        for (int j = 0; j < n; j++) c += ((int)D[j] - int_min) == bi;
        if (c > best || (c == best && bi < best_bin)) { best = c; best_bin = bi; }
    }
    for (int i = 1; i < n; i++) {                                            // (insertion sort: n <= 19)
        const double v = D[i];
        int j = i - 1;
        for (; j >= 0 && D[j] > v; j--) D[j + 1] = D[j];
        D[j + 1] = v;
    }
    const int half = n / 2;
    double med = D[half];
    if ((n & 1) == 0) { med += D[half - 1]; med /= 2.0; }
    o[0] = mn; o[1] = mx; o[2] = mean; o[3] = med; o[4] = sd; o[5] = (double)(best_bin + int_min);
}

struct CalShared {
    double W[kCaliperAngles - 1][kMartinLevels];   // Martin: the hull's width at every level of every angle
    double F[kCaliperAngles];                      // Feret: max x - min x per angle
    double M[kCaliperAngles - 1];                  // Martin: the selected width (valid: bit k of m_ok)
    double N[kCaliperAngles - 1];                  // Nassenstein: the chord per angle
    double A[kCaliperAngles];                      // Feret: the angles of the kept diameters
    float red[kCW][4];                             // per wave: min x, max x, min y, max y of the turned vertices
    uint32_t m_skip, m_ok;                         // Martin: angles skipped before the levels (maxY <= minY) | angles with a value
    int n_hull, n_up, n_lo;
    long long sum_x, sum_y;
};

// tab: mn[cap] | mx[cap] | lo[2 cap]  (the turned vertices float2[2 cap] afterwards), up[2 cap] -- LDS or global
template <typename Sweep>
__device__ __forceinline__ void caliper_body(const CalArgs& R, CalShared& S, unsigned char* tab, uint32_t cap, uint32_t w, uint32_t ox,
                                             uint32_t oy, double* row_out, int tid, Sweep&& sweep)
{
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t* const mn = (uint32_t*)tab;
    uint32_t* const mx = mn + cap;
    uint32_t* const lo = mx + cap;
    uint32_t* const up = (uint32_t*)(tab + 16ull * cap);
    float2* const P = (float2*)tab;
    const bool do_fe = (R.fams & NYXHIP_FAM_FERET) != 0, do_ma = (R.fams & NYXHIP_FAM_MARTIN) != 0, do_na = (R.fams & NYXHIP_FAM_NASSENSTEIN) != 0;
    // ---- per-column extremes ------------------------------------------------------------------------------------------------
    for (uint32_t c = (uint32_t)tid; c < w; c += kCB) { mn[c] = kNoPoint; mx[c] = 0u; }
    if (tid == 0) { S.m_skip = 0u; S.m_ok = 0u; }
    __syncthreads();
    sweep([&](uint32_t x, uint32_t y) {
        if (x < w) { atomicMin(&mn[x], y); atomicMax(&mx[x], y); }
    });
    __syncthreads();
    // ---- monotone chain (convex_hull_nontriv.cpp:92-112): points in (x, y) order, popped while !right_turn ----------------------
    if (tid == 0) {
        int nu = 0, nl = 0;
        const int lim = (int)(2u * cap);
        auto push = [&](uint32_t* st, int& m, uint32_t p) {
            while (m > 1 && !right_turn(st[m - 2], st[m - 1], p)) m--;
            if (m < lim) st[m++] = p;
        };
        for (uint32_t c = 0; c < w; c++) {
            const uint32_t a = mn[c], b = mx[c];
            if (a == kNoPoint) continue;
            push(up, nu, c | (a << 16));
            if (b != a) push(up, nu, c | (b << 16));
        }
        for (uint32_t c = w; c-- > 0;) {
            const uint32_t a = mn[c], b = mx[c];
            if (a == kNoPoint) continue;
            if (b != a) push(lo, nl, c | (b << 16));
            push(lo, nl, c | (a << 16));
        }
        S.n_up = nu; S.n_lo = nl;
    }
    __syncthreads();
    // the lower chain's points that the upper chain holds already (:117-119; the points of a chain are distinct)
    {
        const int nu = S.n_up, nl = S.n_lo;
        for (int j = tid; j < nl; j += kCB) {
            const uint32_t p = lo[j];
            bool found = false;
            for (int i = 0; i < nu && !found; i++) found = up[i] == p;
            if (found) lo[j] = kNoPoint;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int nh = S.n_up;
        const int nl = S.n_lo, lim = (int)(2u * cap);
        for (int j = 0; j < nl; j++)
            if (lo[j] != kNoPoint && nh < lim) up[nh++] = lo[j];
        long long sx = 0, sy = 0;
        for (int i = 0; i < nh; i++) { sx += up[i] & 0xFFFFu; sy += up[i] >> 16; }
        S.n_hull = nh; S.sum_x = sx + (long long)nh * ox; S.sum_y = sy + (long long)nh * oy;
    }
    __syncthreads();
    const int nh = S.n_hull;
    const double cx = (double)S.sum_x / (double)nh, cy = (double)S.sum_y / (double)nh;
    // ---- the angles ---------------------------------------------------------------------------------------------------------
    for (int k = 0; k < kCaliperAngles; k++) {
        if (k == kCaliperAngles - 1 && !do_fe)
            break;                                                           // (theta = 180: Feret only)
        const double sn = R.sn[k], cs = R.cs[k];
        float x0 = 0.f, x1 = 0.f, y0 = 0.f, y1 = 0.f;
        bool first = true;
        for (int i = tid; i < nh; i += kCB) {
            const uint32_t p = up[i];
            const double px = (double)((long long)(p & 0xFFFFu) + (long long)ox), py = (double)((long long)(p >> 16) + (long long)oy);
            const double xr = (px - cx) * cs - (py - cy) * sn + cx;
            const double yr = (py - cy) * cs + (px - cx) * sn + cy;
            const float xf = (float)xr, yf = (float)yr;
            P[i] = make_float2(xf, yf);
            if (first) { x0 = x1 = xf; y0 = y1 = yf; first = false; }
            else { x0 = xf < x0 ? xf : x0; x1 = x1 < xf ? xf : x1; y0 = yf < y0 ? yf : y0; y1 = y1 < yf ? yf : y1; }
        }
        // (lanes without a vertex take a neighbour's values: thread 0 always has one)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ax0 = __shfl_xor(x0, o, 64), ax1 = __shfl_xor(x1, o, 64), ay0 = __shfl_xor(y0, o, 64), ay1 = __shfl_xor(y1, o, 64);
            const bool of = __shfl_xor((int)first, o, 64) != 0;
            if (!of) {
                if (first) { x0 = ax0; x1 = ax1; y0 = ay0; y1 = ay1; first = false; }
                else { x0 = ax0 < x0 ? ax0 : x0; x1 = x1 < ax1 ? ax1 : x1; y0 = ay0 < y0 ? ay0 : y0; y1 = y1 < ay1 ? ay1 : y1; }
            }
        }
        if (lane == 0) {
            if (first) { x0 = y0 = __int_as_float(0x7f800000); x1 = y1 = __int_as_float(0xff800000); }   // a wave without vertices
            S.red[wave][0] = x0; S.red[wave][1] = x1; S.red[wave][2] = y0; S.red[wave][3] = y1;
        }
        __syncthreads();
        float fx0 = S.red[0][0], fx1 = S.red[0][1], fy0 = S.red[0][2], fy1 = S.red[0][3];
#pragma unroll
        for (int q = 1; q < kCW; q++) {
            fx0 = S.red[q][0] < fx0 ? S.red[q][0] : fx0; fx1 = fx1 < S.red[q][1] ? S.red[q][1] : fx1;
            fy0 = S.red[q][2] < fy0 ? S.red[q][2] : fy0; fy1 = fy1 < S.red[q][3] ? S.red[q][3] : fy1;
        }
        if (tid == 0) S.F[k] = (double)fx1 - (double)fx0;
        if (k < kCaliperAngles - 1) {
            if (do_ma) {
                const double min_y = fy0, max_y = fy1;
                if (max_y <= min_y) {
                    if (tid == 0) S.m_skip |= 1u << k;
                } else if (tid < kMartinLevels) {
                    const double step = (max_y - min_y) / (double)kMartinLevels;
                    S.W[k][tid] = span_at<true>(P, nh, min_y + ((double)tid + 0.5) * step);
                }
            }
            if (do_na && nh >= 3 && tid == 2 * 64) {
                const double ymax = fy1;
                double xsum = 0.0;
                int cnt = 0;
                for (int i = 0; i < nh; i++) {
                    const float2 q = P[i];
                    if (fabs((double)q.y - ymax) < 1e-3) { xsum += (double)q.x; cnt++; }
                }
                S.N[k] = span_at<false>(P, nh, xsum / (double)(cnt > 1 ? cnt : 1));
            }
        }
        __syncthreads();
    }
    // ---- Martin: the width at the level that halves the summed widths (caliper_martin.cpp:121-135) ------------------------------
    if (do_ma && tid < kCaliperAngles - 1 && !((S.m_skip >> tid) & 1u)) {
        const double* wd = S.W[tid];
        double total = 0.0;
        for (int i = 0; i < kMartinLevels; i++) total += wd[i];
        if (total > 0.0) {
            const double half = 0.5 * total;
            double cum = 0.0, m = wd[kMartinLevels - 1];
            for (int i = 0; i < kMartinLevels; i++) {
                cum += wd[i];
                if (cum >= half) { m = wd[i]; break; }
            }
            S.M[tid] = m;
            atomicOr(&S.m_ok, 1u << tid);
        }
    }
    __syncthreads();
    // ---- statistics: one lane per class, each in a wave of its own -----------------------------------------------------------------
    if (do_fe && tid == 0) {
        int m = 0;
        for (int k = 0; k < kCaliperAngles; k++) {
            const double f = S.F[k];
            if (f > 0.0) { S.F[m] = f; S.A[m] = (double)(10 * k); m++; }     // (m <= k: in place)
        }
        double* o = row_out + R.col_feret;
        if (m == 0) {
            for (int i = 0; i < kFeretCols; i++) o[i] = R.soft_nan;
        } else {
            int i_min = 0, i_max = 0;                                        // get_minmax_idx: the first minimum, the first maximum
            for (int i = 1; i < m; i++) {
                if (S.F[i] < S.F[i_min]) i_min = i;
                if (S.F[i] > S.F[i_max]) i_max = i;
            }
            o[0] = S.A[i_min]; o[1] = S.A[i_max];
            common_stats(S.F, m, o + 2);
        }
    }
    if (do_ma && tid == 64) {
        int m = 0;
        const uint32_t ok = S.m_ok;
        for (int k = 0; k < kCaliperAngles - 1; k++)
            if ((ok >> k) & 1u) S.M[m++] = S.M[k];
        common_stats(S.M, m, row_out + R.col_martin);
    }
    if (do_na && tid == 128)
        common_stats(S.N, nh >= 3 ? kCaliperAngles - 1 : 0, row_out + R.col_nassenstein);
}

} // namespace

__global__ __launch_bounds__(kCB) void roi_caliper_kernel(const CalArgs R)
{
    __shared__ CalShared S;
    extern __shared__ __attribute__((aligned(16))) unsigned char cal_lds[];   // [kCaliperBytesPerCol * R.cols_cap]
    const int tid = threadIdx.x;
    const uint64_t roi = R.roi_index ? R.roi_index[blockIdx.x] : blockIdx.x;
    if (roi >= R.n_roi)
        return;
    const uint64_t off = R.px_offset[roi];
    const uint32_t n = (uint32_t)(R.px_offset[roi + 1] - off);
    const uint32_t w = R.bbox_w[roi];
    double* const row_out = R.out + roi * R.ld;
    auto fill_row = [&](double v) {
        if (tid != 0) return;
        if (R.fams & NYXHIP_FAM_FERET) for (int i = 0; i < kFeretCols; i++) row_out[R.col_feret + i] = v;
        if (R.fams & NYXHIP_FAM_MARTIN) for (int i = 0; i < kMartinCols; i++) row_out[R.col_martin + i] = v;
        if (R.fams & NYXHIP_FAM_NASSENSTEIN) for (int i = 0; i < kNassensteinCols; i++) row_out[R.col_nassenstein + i] = v;
    };
    const bool wide = w > R.cols_cap;
    if (wide) {
        if (R.defer_wide)
            return;                                                          // served by the launch over the list of such ROIs
        if (!R.ws || w > R.ws_cols) {                                        // (a box beyond what the caller stated)
            if (tid == 0) atomicCAS(R.status, 0, NYXHIP_ERR_ROI_TOO_LARGE);
            fill_row(__longlong_as_double(0x7ff8000000000000LL));
            return;
        }
    }
    if (n < 2) { fill_row(R.soft_nan); return; }                             // no hull (build_convex_hull: cloud.size() < 2)
    const uint32_t ox = R.origin_x ? R.origin_x[roi] : 0u, oy = R.origin_y ? R.origin_y[roi] : 0u;
    const uint16_t* const xs = R.x + off;
    const uint16_t* const ys = R.y + off;
    auto sweep = [&](auto&& f) {
        for (uint32_t i = (uint32_t)tid; i < n; i += kCB) f((uint32_t)xs[i], (uint32_t)ys[i]);
    };
    if (wide) caliper_body(R, S, R.ws + (uint64_t)blockIdx.x * kCaliperBytesPerCol * R.ws_cols, R.ws_cols, w, ox, oy, row_out, tid, sweep);
    else caliper_body(R, S, cal_lds, R.cols_cap, w, ox, oy, row_out, tid, sweep);
}

__device__ bool CaliperWide::operator()(uint64_t i, uint32_t*) const
{
    return bw[i] > cap;
}
template int deferred_classify<CaliperWide>(uint64_t, const CaliperWide&, uint32_t*, hipStream_t);

int launch_roi_caliper(const CalArgs& a, void* stream, uint32_t grid)
{
    if (grid == 0)
        return 0;
    const uint32_t dyn = kCaliperBytesPerCol * a.cols_cap;                   // (<= 24 KiB)
    hipLaunchKernelGGL(roi_caliper_kernel, dim3(grid), dim3(kCB), dyn, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace nyxhip
