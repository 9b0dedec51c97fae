// roi_circle.hip -- two classes of the reference's shape block that read the ROI's merged contour at its ABSOLUTE position:
//   EnclosingInscribingCircumscribingCircleFeature  DIAMETER_MIN_ENCLOSING_CIRCLE, DIAMETER_CIRCUMSCRIBING_CIRCLE,
//                                                   DIAMETER_INSCRIBING_CIRCLE          features/circle.cpp:28-244 (of the reference)
//   GeodeticLengthThicknessFeature                  GEODETIC_LENGTH, THICKNESS          features/geo_len_thickness.cpp:22-35
//
//   roi_circle_kernel   The fourth reader of the contour roi_contour_kernel left in the workspace.  A wave per ROI, kCircleWaves ROIs per
//                       workgroup (the waves never meet: no workgroup barrier).  The contour stays in its packed x | y << 16 form: in
//                       the wave's LDS slot when it has at most MomArgs::k_cap points, in the workspace otherwise.  A contour point
//                       of the reference is padded + origin in integers (contour.cpp:673-679); that integer is formed first and
//                       converted where the reference converts it.
//                       Centroid   integer sums of the cloud in 64 bits + n * origin, one conversion and one division per axis
//                                  (basic_morphology.cpp:40-47: the sequential fp64 sum is exact below 2^53).
//                       Radii      per contour point sqrt(tx * tx + ty * ty), tx = x - (cx - 1), fp64, unfused; wave maximum / minimum.
//                       Perimeter  sqrt((double) sqdist) per consecutive pair (term 0: last point to first), the terms computed 64
//                                  at a time and ADDED ONE AFTER THE OTHER in the reference's order (contour.cpp:960-974): the sum
//                                  decides the branch SqRootTmp < 0.
//                       Enclosing  the reference's incremental three-level search in float (circle.cpp:87-173).  Centre and radius
//                                  are wave-uniform; each of the three nested scans is "every lane tests its point, ballot, first
//                                  set bit, one uniform update, go on behind that point" -- the per-point test has no state but
//                                  centre and radius, so these are the reference's decisions in the reference's order.
//   Float numerics: products and sums are separate instructions (-ffp-contract=off).  Float division and square root are taken in
//   fp64 and rounded to float once: for these two operations double rounding from 53 to 24 bits is innocuous (53 >= 2 * 24 + 2), so
//   the result is the correctly rounded float whatever the float instructions of the device do; fp64 division and square root are
//   correctly rounded.  Integers become floats through fp64 as well (exact below 2^53, then one rounding).
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_circle.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

constexpr float kCircEps = 1.0e-4f;                                           // circle.h:54

__device__ __forceinline__ float f32_of(long long v) { return (float)(double)v; }
__device__ __forceinline__ float f32_sqrt(float v) { return (float)sqrt((double)v); }
__device__ __forceinline__ float f32_div(float a, float b) { return (float)((double)a / (double)b); }
// Point2f::normL2 (pixel.h:23)
__device__ __forceinline__ float norm_l2(float dx, float dy) { return f32_sqrt(dx * dx + dy * dy); }
// Pixel2::operator/ (2.0f) and operator* (0.5f), then operator Point2f: (float) StatsInt((float) v / 2.0f) -- halving a float is exact
__device__ __forceinline__ float trunc_half(long long v) { return truncf(f32_of(v) * 0.5f); }

struct Circ { float cx, cy, r; };

// findCircle3pts (circle.cpp:42-85)
__device__ __forceinline__ Circ circle3(long long x0, long long y0, long long x1, long long y1, long long x2, long long y2)
{
    const float v1x = f32_of(x1 - x0), v1y = f32_of(y1 - y0), v2x = f32_of(x2 - x0), v2y = f32_of(y2 - y0);
    const float c1 = trunc_half(x0 + x1) * v1x + trunc_half(y0 + y1) * v1y;
    const float c2 = trunc_half(x0 + x2) * v2x + trunc_half(y0 + y2) * v2y;
    const float det = v1x * v2y - v1y * v2x;
    Circ c;
    if (fabsf(det) <= kCircEps) {
        // (collinear) "squared distances" that are distances, rooted again; sqrt, * 0.5f and + EPS are the reference's double ones
        const float d1 = norm_l2(f32_of(x0 - x1), f32_of(y0 - y1)), d2 = norm_l2(f32_of(x0 - x2), f32_of(y0 - y2)),
                    d3 = norm_l2(f32_of(x1 - x2), f32_of(y1 - y2));
        const float mx = fmaxf(d1, fmaxf(d2, d3));
        c.r = (float)(sqrt((double)mx) * 0.5 + (double)kCircEps);
        if (d1 >= d2 && d1 >= d3) { c.cx = trunc_half(x0 + x1); c.cy = trunc_half(y0 + y1); }
        else if (d2 >= d1 && d2 >= d3) { c.cx = trunc_half(x0 + x2); c.cy = trunc_half(y0 + y2); }
        else { c.cx = trunc_half(x1 + x2); c.cy = trunc_half(y1 + y2); }
        return c;
    }
    c.cx = f32_div(c1 * v2y - c2 * v1y, det);
    c.cy = f32_div(v1x * c2 - v2x * c1, det);
    const float ex = c.cx - f32_of(x0), ey = c.cy - f32_of(y0);
    c.r = f32_sqrt(ex * ex + ey * ey) + kCircEps;
    return c;
}

// The work of one wave on one ROI.  K: the contour, in LDS or in the workspace (the caller passes the array itself so that the
// accesses keep their address space).
template <typename KP>
__device__ __forceinline__ void circle_body(const CircArgs& R, KP K, int nK, uint64_t off, uint32_t n, long long ox, long long oy, double* row_out, int lane)
{
    const MomArgs& A = R.m;
    auto px_of = [&](int i) -> long long { return (long long)(K[i] & 0xFFFFu) + ox; };
    auto py_of = [&](int i) -> long long { return (long long)(K[i] >> 16) + oy; };
    if (R.fams & NYXHIP_FAM_GEODETIC) {
        double per = 0.0;
        for (int base = 0; base < nK; base += 64) {
            const int i = base + lane;
            double term = 0.0;
            if (i < nK) {
                const uint32_t p = K[i], q = K[i == 0 ? nK - 1 : i - 1];
                const long long dx = (long long)(p & 0xFFFFu) - (long long)(q & 0xFFFFu), dy = (long long)(p >> 16) - (long long)(q >> 16);
                term = sqrt((double)(dx * dx + dy * dy));
            }
            const int cnt = min(64, nK - base);
            for (int t = 0; t < cnt; t++) per += __shfl(term, t, 64);         // the reference's order: one dependent add per point
        }
        if (lane == 0) {
            double sq = per * per / 16.0 - (double)n;                         // geo_len_thickness.cpp:22-35; area = the pixel count
            if (sq < 0) sq = 0;
            const double gl = per / 4.0 + sqrt(sq);
            row_out[R.col_geodetic] = gl;
            row_out[R.col_geodetic + 1] = per / 2.0 - gl;
        }
    }
    if (!(R.fams & NYXHIP_FAM_CIRCLES))
        return;
    if (nK == 0) {                                                            // circle.cpp:257: skipped, the initial zeros stay
        if (lane < kCirclesCols) row_out[R.col_circles + lane] = 0.0;
        return;
    }
    // ---- centroid (basic_morphology.cpp:40-47) ------------------------------------------------------------------------------
    unsigned long long sx = 0, sy = 0;
    for (uint32_t i = (uint32_t)lane; i < n; i += 64) { sx += A.x[off + i]; sy += A.y[off + i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); }
    const double cen_x = (double)(sx + (unsigned long long)n * (unsigned long long)ox) / (double)n;
    const double cen_y = (double)(sy + (unsigned long long)n * (unsigned long long)oy) / (double)n;
    // ---- circumscribing / inscribing (circle.cpp:220-244) ---------------------------------------------------------------------
    {
        const double x2 = cen_x - 1.0, y2 = cen_y - 1.0;
        double dmax = 0.0, dmin = __longlong_as_double(0x7ff0000000000000LL);
        for (int i = lane; i < nK; i += 64) {
            const double tx = (double)px_of(i) - x2, ty = (double)py_of(i) - y2;
            const double d = sqrt(tx * tx + ty * ty);
            dmax = d > dmax ? d : dmax;
            dmin = d < dmin ? d : dmin;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double a = __shfl_xor(dmax, o, 64), b = __shfl_xor(dmin, o, 64);
            dmax = a > dmax ? a : dmax;
            dmin = b < dmin ? b : dmin;
        }
        if (lane == 0) { row_out[R.col_circles + 1] = 2.0 * dmax; row_out[R.col_circles + 2] = 2.0 * dmin; }
    }
    // ---- minimum enclosing circle (circle.cpp:145-217) ------------------------------------------------------------------------
    float radius;
    if (nK == 1)
        radius = kCircEps;
    else if (nK == 2) {
        const float ax = f32_of(px_of(0)), ay = f32_of(py_of(0)), bx = f32_of(px_of(1)), by = f32_of(py_of(1));
        radius = (float)((double)norm_l2(ax - bx, ay - by) / 2.0) + kCircEps;
    } else {
        // first index of [lo, hi) whose point is not strictly inside the circle, or hi (wave-uniform)
        auto first_out = [&](int lo, int hi, const Circ& c) -> int {
            for (int base = lo; base < hi; base += 64) {
                const int i = base + lane;
                bool out = false;
                if (i < hi) {
                    const float dx = c.cx - f32_of(px_of(i)), dy = c.cy - f32_of(py_of(i));
                    out = !(norm_l2(dx, dy) < c.r);
                }
                const unsigned long long b = __ballot(out);
                if (b)
                    return __builtin_amdgcn_readfirstlane(base + __ffsll((long long)b) - 1);
            }
            return hi;
        };
        // the circle on two points as its diameter (circle.cpp:89-93, :120-124, :147-151)
        auto two_point = [&](int a, int b) -> Circ {
            const long long xa = px_of(a), ya = py_of(a), xb = px_of(b), yb = py_of(b);
            Circ c;
            c.cx = f32_of(xa + xb) / 2.0f;
            c.cy = f32_of(ya + yb) / 2.0f;
            c.r = norm_l2(f32_of(xa - xb), f32_of(ya - yb)) / 2.0f + kCircEps;
            return c;
        };
        Circ c1 = two_point(0, 1);
        for (int i = 2;; i++) {
            i = first_out(i, nK, c1);
            if (i >= nK) break;
            Circ c2 = two_point(0, i);                                        // findSecondPoint
            for (int j = 1;; j++) {
                j = first_out(j, i, c2);
                if (j >= i) break;
                Circ c3 = two_point(j, i);                                    // findThirdPoint
                for (int k = 0;; k++) {
                    k = first_out(k, j, c3);
                    if (k >= j) break;
                    const Circ nc = circle3(px_of(i), py_of(i), px_of(j), py_of(j), px_of(k), py_of(k));
                    if (nc.r > 0) c3 = nc;
                }
                if (c3.r > 0) c2 = c3;
            }
            if (c2.r > 0) c1 = c2;
        }
        radius = c1.r;
    }
    if (lane == 0) row_out[R.col_circles] = (double)(2.0f * radius);
}

} // namespace

__global__ __launch_bounds__(64 * kCircleWaves) void roi_circle_kernel(const CircArgs R)
{
    const MomArgs& A = R.m;
    extern __shared__ __attribute__((aligned(16))) unsigned char circ_lds[];
    const int lane = threadIdx.x & 63, wslot = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t slot = (uint64_t)blockIdx.x * kCircleWaves + (uint64_t)wslot;
    if (slot >= R.grid_rois)
        return;
    const uint64_t roi = A.sp.roi_index ? A.sp.roi_index[slot] : slot;       // (a list: the big boxes of a batch)
    if (roi >= A.n_roi)
        return;
    const uint64_t off = A.px_offset[roi];
    const uint32_t n = (uint32_t)(A.px_offset[roi + 1] - off);
    const uint32_t bw_ = A.bbox_w[roi], bh_ = A.bbox_h[roi];
    if (A.sp.defer_large && (uint64_t)(bw_ + 2u) * (bh_ + 2u) > A.plane_cap)
        return;                                                               // served by the launch over the big-box list
    double* const row_out = A.out + roi * A.ld;
    if (n == 0) {                                                             // a blank ROI: zeros, as the outline kernel writes them
        if ((R.fams & NYXHIP_FAM_CIRCLES) && lane < kCirclesCols) row_out[R.col_circles + lane] = 0.0;
        if ((R.fams & NYXHIP_FAM_GEODETIC) && lane < kGeodeticCols) row_out[R.col_geodetic + lane] = 0.0;
        return;
    }
    const int nK = __builtin_amdgcn_readfirstlane((int)A.n_contour[roi]);
    const long long ox = R.origin_x ? (long long)R.origin_x[roi] : 0, oy = R.origin_y ? (long long)R.origin_y[roi] : 0;
    const uint32_t* const Kg = A.ws_contour + off;
    if (nK <= (int)A.k_cap) {
        uint32_t* const s_K = (uint32_t*)circ_lds + (size_t)wslot * A.k_cap;
        for (int i = lane; i < nK; i += 64) s_K[i] = Kg[i];
        wav_sync<false>();
        circle_body(R, s_K, nK, off, n, ox, oy, row_out, lane);
    } else
        circle_body(R, Kg, nK, off, n, ox, oy, row_out, lane);
}

int launch_roi_circle(const CircArgs& a, void* stream, uint32_t grid)
{
    if (grid == 0)
        return 0;
    CircArgs b = a;
    b.grid_rois = grid;
    const uint32_t dyn = (uint32_t)kCircleWaves * 4u * a.m.k_cap;             // (<= 32 KiB)
    hipLaunchKernelGGL(roi_circle_kernel, dim3((grid + kCircleWaves - 1) / kCircleWaves), dim3(64 * kCircleWaves), dyn, (hipStream_t)stream, b);
    return (int)hipGetLastError();
}

} // namespace nyxhip
