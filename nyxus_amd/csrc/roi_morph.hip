// roi_morph.hip -- four classes of the reference's 2-D shape block, behind the morphology entries (nyxhip_morph.hip):
//   BasicMorphologyFeatures  AREA_PIXELS_COUNT .. ASPECT_RATIO (15)                 features/basic_morphology.cpp:19-92 (of the reference)
//   ContourFeature           PERIMETER .. EDGE_INTEGRATED_INTENSITY (7)            features/contour.cpp:935-1021
//   ConvexHullFeature        CIRCULARITY, CONVEX_HULL_AREA, SOLIDITY               features/convex_hull_nontriv.cpp:18-33, :53-120, :193-213
//   ExtremaFeature           EXTREMA_P1_X .. EXTREMA_P8_Y (16)                     features/extrema.cpp:15-74
//
//   roi_morph_kernel   One 256-thread workgroup per ROI, all four classes fused: the cloud is read once for the integer sums, the packed
//                      extrema keys, the per-column extremes and the intensity plane, and twice more (coordinates only) for the distance
//                      moments of COMPACTNESS.
//                      Sweep 1   sum x, sum y, sum I in 64 bits; sum x I and sum y I as two 64-bit sums each, over the low and the high
//                                half of the intensity (x < 2^16, half < 2^16, n < 2^32: no sum wraps); eight packed keys whose minimum /
//                                maximum are the eight extrema; min / max y of every box column (integer atomics); the intensity at its
//                                cell of a dense u32 plane.  Tables and plane live in LDS up to MorphArgs::cols_cap / plane_cap and in a
//                                global block per workgroup beyond (a list launch, deferred_list.h).  The plane is not cleared: it is
//                                read at contour points only, and a contour point is a pixel of the cloud.
//                      Sweeps 2, 3  the distances to the centroid: their mean, then their centred sum of squares, both added as
//                                fixed-point integers (57 bits below the largest possible term), so neither depends on the pixel order.
//                      Hull      one lane: the reference's monotone chain over the <= 2 w column extremes in (x, y) order, popping while
//                                !right_turn, the lower chain's new points appended (the construction of roi_caliper.hip, restated: that
//                                kernel stays as it is).  2 A + B -- shoelace sum and lattice points on the edges -- is one integer.
//                      Contour   wave 0 adds the perimeter's terms one after the other in the reference's order (roi_circle.hip:82-92,
//                                restated); all threads gather the plane at the contour's points: integer sum, minimum, maximum, then
//                                the centred sum of squares about sum / count.
//   Every sum that decides a bit is an integer or a fixed sequence of fp64 operations: a row depends neither on scheduling nor on the
//   path (LDS / global) nor on which classes share the call.  Built with -ffp-contract=off like every unit.
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_morph.h"
#include "launch_util.h"
#include "deferred_list.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

constexpr int kMB = 256;
constexpr int kMW = kMB / 64;
constexpr uint32_t kNoPoint = 0xFFFFFFFFu;    // (a box is at most 65535 wide: x = 65535 does not occur)
constexpr double kPi = 3.14159265358979323846;   // M_PI

// ConvexHullFeature::right_turn on points x | y << 16
__device__ __forceinline__ bool right_turn(uint32_t p1, uint32_t p2, uint32_t p3)
{
    const long long x1 = p1 & 0xFFFFu, y1 = p1 >> 16, x2 = p2 & 0xFFFFu, y2 = p2 >> 16, x3 = p3 & 0xFFFFu, y3 = p3 >> 16;
    return (x3 - x1) * (y2 - y1) - (y3 - y1) * (x2 - x1) > 0;
}

// (Euclid on two 16-bit values: at most 24 steps)
__device__ __forceinline__ uint32_t gcd_u32(uint32_t a, uint32_t b)
{
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    return a;
}

// the correctly rounded double of a 128-bit integer: 64 leading bits and a sticky bit, one rounding, an exact scaling
__device__ __forceinline__ double f64_of_u128(unsigned __int128 v)
{
    const unsigned long long hi = (unsigned long long)(v >> 64);
    if (hi == 0) return (double)(unsigned long long)v;
    const int s = 64 - __clzll((long long)hi);                               // 1 .. 64
    unsigned long long top = (unsigned long long)(v >> s);
    if ((v & ((((unsigned __int128)1) << s) - 1)) != 0) top |= 1ull;
    return ldexp((double)top, s);
}

struct MorphShared {
    unsigned long long sx, sy, sI, sxIlo, sxIhi, syIlo, syIhi;   // sweep 1
    unsigned long long eS;                                        // sum of the contour points' intensities
    unsigned long long twoA, B;                                   // hull: shoelace sum (two's complement), lattice points on the edges
    unsigned long long fx[2], dmin, dmax;                         // fixed-point distance sums (low / high halves); bit patterns of the extreme distances
    uint32_t key[8];                                              // packed extrema keys: 0, 1, 6, 7 minima; 2 .. 5 maxima
    uint32_t eMin, eMax;
    int n_up, n_lo, n_hull;
    double red[kMW];
    double per;
};

// sum over the workgroup in a fixed order; every thread gets it (two barriers)
__device__ __forceinline__ double block_sum(double v, MorphShared& S, int tid)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((tid & 63) == 0) S.red[tid >> 6] = v;
    __syncthreads();
    const double t = ((S.red[0] + S.red[1]) + S.red[2]) + S.red[3];
    __syncthreads();
    return t;
}

__device__ __forceinline__ unsigned long long wave_add(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64); v = u < v ? u : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64); v = u > v ? u : v; }
    return v;
}

// tab: mn[cap] | mx[cap] | lo[2 cap] | up[2 cap] (LDS or global); plane: u32[w * h] (LDS or global).  n >= 1.
__device__ __forceinline__ void morph_body(const MorphArgs& R, MorphShared& S, unsigned char* tab, uint32_t cap, uint32_t* plane, uint64_t off,
                                           uint32_t n, uint32_t w, uint32_t h, unsigned long long ox, unsigned long long oy, const uint32_t* K, int nK,
                                           double* row_out, int tid)
{
    const int lane = tid & 63;
    const bool do_basic = (R.morph & NYXHIP_MORPH_BASIC) != 0, do_con = (R.morph & NYXHIP_MORPH_CONTOUR) != 0,
               do_hull = (R.morph & NYXHIP_MORPH_HULL) != 0, do_ext = (R.morph & NYXHIP_MORPH_EXTREMA) != 0;
    uint32_t* const mn = (uint32_t*)tab;
    uint32_t* const mx = mn + cap;
    uint32_t* const lo = mx + cap;
    uint32_t* const up = lo + 2ull * cap;
    const uint16_t* const xs = R.x + off;
    const uint16_t* const ys = R.y + off;
    const uint32_t* const vs = R.inten + off;
    // ---- sweep 1 ------------------------------------------------------------------------------------------------------------
    if (do_hull)
        for (uint32_t c = (uint32_t)tid; c < w; c += kMB) { mn[c] = kNoPoint; mx[c] = 0u; }
    if (tid == 0) {
        S.sx = S.sy = S.sI = S.sxIlo = S.sxIhi = S.syIlo = S.syIhi = S.eS = S.twoA = S.B = 0ull;
        S.key[0] = S.key[1] = S.key[6] = S.key[7] = 0xFFFFFFFFu;
        S.key[2] = S.key[3] = S.key[4] = S.key[5] = 0u;
        S.eMin = 0xFFFFFFFFu; S.eMax = 0u;
        S.fx[0] = S.fx[1] = 0ull; S.dmin = ~0ull; S.dmax = 0ull;
        S.n_up = S.n_lo = S.n_hull = 0;
        S.per = 0.0;
    }
    __syncthreads();
    {
        unsigned long long sx = 0, sy = 0, sI = 0, xl = 0, xh = 0, yl = 0, yh = 0;
        uint32_t k0 = 0xFFFFFFFFu, k1 = 0xFFFFFFFFu, k2 = 0, k3 = 0, k4 = 0, k5 = 0, k6 = 0xFFFFFFFFu, k7 = 0xFFFFFFFFu;
        bool outside = false;
        for (uint32_t i = (uint32_t)tid; i < n; i += kMB) {
            const uint32_t x = xs[i], y = ys[i], v = vs[i];
            if (x >= w || y >= h) { outside = true; continue; }              // never stored, never counted: the call fails
            sx += x; sy += y; sI += v;
            const unsigned long long vl = v & 0xFFFFu, vh = v >> 16;
            xl += x * vl; xh += x * vh; yl += y * vl; yh += y * vh;
            const uint32_t yx = y << 16 | x, ynx = y << 16 | (0xFFFFu - x), xy = x << 16 | y, xny = x << 16 | (0xFFFFu - y);
            k0 = yx < k0 ? yx : k0;        // P1: the top row's leftmost pixel
            k1 = ynx < k1 ? ynx : k1;      // P2: the top row's rightmost
            k2 = xny > k2 ? xny : k2;      // P3: the right column's top
            k3 = xy > k3 ? xy : k3;        // P4: the right column's bottom
            k4 = yx > k4 ? yx : k4;        // P5: the bottom row's rightmost
            k5 = ynx > k5 ? ynx : k5;      // P6: the bottom row's leftmost
            k6 = xny < k6 ? xny : k6;      // P7: the left column's bottom
            k7 = xy < k7 ? xy : k7;        // P8: the left column's top
            if (do_hull) { atomicMin(&mn[x], y); atomicMax(&mx[x], y); }
            if (do_con) plane[(size_t)y * w + x] = v;
        }
        if (__any(outside) && lane == 0) atomicCAS(R.status, 0, NYXHIP_ERR_INVALID_ARG);
        sx = wave_add(sx); sy = wave_add(sy); sI = wave_add(sI);
        xl = wave_add(xl); xh = wave_add(xh); yl = wave_add(yl); yh = wave_add(yh);
        k0 = wave_min(k0); k1 = wave_min(k1); k6 = wave_min(k6); k7 = wave_min(k7);
        k2 = wave_max(k2); k3 = wave_max(k3); k4 = wave_max(k4); k5 = wave_max(k5);
        if (lane == 0) {
            atomicAdd(&S.sx, sx); atomicAdd(&S.sy, sy); atomicAdd(&S.sI, sI);
            atomicAdd(&S.sxIlo, xl); atomicAdd(&S.sxIhi, xh); atomicAdd(&S.syIlo, yl); atomicAdd(&S.syIhi, yh);
            atomicMin(&S.key[0], k0); atomicMin(&S.key[1], k1); atomicMin(&S.key[6], k6); atomicMin(&S.key[7], k7);
            atomicMax(&S.key[2], k2); atomicMax(&S.key[3], k3); atomicMax(&S.key[4], k4); atomicMax(&S.key[5], k5);
        }
    }
    __syncthreads();
    // ---- extrema (extrema.cpp:58-73) ------------------------------------------------------------------------------------------
    if (do_ext && tid < 8) {
        const uint32_t k = S.key[tid];
        uint32_t x, y;
        switch (tid) {
        case 0: case 4: x = k & 0xFFFFu; y = k >> 16; break;                 // y << 16 | x
        case 1: case 5: x = 0xFFFFu - (k & 0xFFFFu); y = k >> 16; break;     // y << 16 | ~x
        case 3: case 7: x = k >> 16; y = k & 0xFFFFu; break;                 // x << 16 | y
        default: x = k >> 16; y = 0xFFFFu - (k & 0xFFFFu); break;            // x << 16 | ~y
        }
        row_out[R.col_extrema + 2 * tid] = (double)(ox + x);
        row_out[R.col_extrema + 2 * tid + 1] = (double)(oy + y);
    }
    // ---- basic morphology (basic_morphology.cpp:19-92) ------------------------------------------------------------------------
    if (do_basic) {
        const double dn = (double)n;
        const double cen_x = (double)(S.sx + (unsigned long long)n * ox) / dn, cen_y = (double)(S.sy + (unsigned long long)n * oy) / dn;
        // The distance moments in FIXED POINT, so that they depend neither on the pixel order nor on scheduling: a term t < 2^k is
        // rounded to a multiple of 2^(k - 57) and the integers are added in two 64-bit sums over their halves (n < 2^32 terms).
        // Sweep 2: sum d at the scale of the box (d < w + h), with the smallest and the largest distance (bit patterns of
        // non-negative doubles order like the integers).  Sweep 3: sum (d - mean)^2 at the scale of the largest deviation.
        const int sh1 = 57 - (32 - __clz(w + h));                            // w + h < 2^(32 - clz)
        unsigned long long qlo = 0, qhi = 0, dlo = ~0ull, dhi = 0ull;
        for (uint32_t i = (uint32_t)tid; i < n; i += kMB) {
            const double dx = (double)(ox + xs[i]) - cen_x, dy = (double)(oy + ys[i]) - cen_y;
            const double d = sqrt(dx * dx + dy * dy);
            const unsigned long long q = (unsigned long long)rint(ldexp(d, sh1)), bits = (unsigned long long)__double_as_longlong(d);
            qlo += q & 0xFFFFFFFFull; qhi += q >> 32;
            dlo = bits < dlo ? bits : dlo; dhi = bits > dhi ? bits : dhi;
        }
        qlo = wave_add(qlo); qhi = wave_add(qhi);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long a = __shfl_xor(dlo, o, 64), b = __shfl_xor(dhi, o, 64);
            dlo = a < dlo ? a : dlo; dhi = b > dhi ? b : dhi;
        }
        if (lane == 0) { atomicAdd(&S.fx[0], qlo); atomicAdd(&S.fx[1], qhi); atomicMin(&S.dmin, dlo); atomicMax(&S.dmax, dhi); }
        __syncthreads();
        const double mean = ldexp(f64_of_u128(((unsigned __int128)S.fx[1] << 32) + S.fx[0]), -sh1) / dn;
        const double e_lo = mean - __longlong_as_double((long long)S.dmin), e_hi = __longlong_as_double((long long)S.dmax) - mean;
        // |d - mean| <= max(|e_lo|, |e_hi|) for every pixel (a rounded mean may lie a rounding outside [d_min, d_max]: hence the fabs)
        const double e_max = fabs(e_lo) > fabs(e_hi) ? fabs(e_lo) : fabs(e_hi), e_max2 = e_max * e_max;
        __syncthreads();
        if (tid == 0) S.fx[0] = S.fx[1] = 0ull;
        __syncthreads();
        double m2 = 0.0;
        if (e_max2 > 0.0) {
            const int sh2 = 56 - ilogb(e_max2);                              // e^2 <= e_max2 < 2^(ilogb + 1)
            qlo = qhi = 0;
            for (uint32_t i = (uint32_t)tid; i < n; i += kMB) {
                const double dx = (double)(ox + xs[i]) - cen_x, dy = (double)(oy + ys[i]) - cen_y;
                const double e = sqrt(dx * dx + dy * dy) - mean;
                const unsigned long long q = (unsigned long long)rint(ldexp(e * e, sh2));
                qlo += q & 0xFFFFFFFFull; qhi += q >> 32;
            }
            qlo = wave_add(qlo); qhi = wave_add(qhi);
            if (lane == 0) { atomicAdd(&S.fx[0], qlo); atomicAdd(&S.fx[1], qhi); }
            __syncthreads();
            m2 = ldexp(f64_of_u128(((unsigned __int128)S.fx[1] << 32) + S.fx[0]), -sh2);
        }
        if (tid == 0) {
            double* const o = row_out + R.col_basic;
            double wcx = 0.0, wcy = 0.0;
            if (S.sI > 0) {
                const unsigned __int128 mass_x = ((unsigned __int128)S.sxIhi << 16) + S.sxIlo + (unsigned __int128)ox * S.sI;
                const unsigned __int128 mass_y = ((unsigned __int128)S.syIhi << 16) + S.syIlo + (unsigned __int128)oy * S.sI;
                const double mass = (double)S.sI;
                wcx = f64_of_u128(mass_x) / mass;
                wcy = f64_of_u128(mass_y) / mass;
            }
            const double ddx = wcx - cen_x, ddy = wcy - cen_y;
            o[0] = dn;                                                        // AREA_PIXELS_COUNT
            o[1] = 0.0;                                                       // AREA_UM2: no XY resolution behind this ABI
            o[2] = cen_x; o[3] = cen_y;
            o[4] = wcy; o[5] = wcx;
            o[6] = sqrt(ddx * ddx + ddy * ddy);                               // MASS_DISPLACEMENT
            o[7] = (n > 2 ? sqrt(m2 / (double)(n - 1)) : 0.0) / dn;           // COMPACTNESS
            o[8] = (double)oy; o[9] = (double)ox;                             // BBOX_YMIN, BBOX_XMIN
            o[10] = (double)h; o[11] = (double)w;                             // BBOX_HEIGHT, BBOX_WIDTH
            o[12] = 2.0 * sqrt(dn / kPi);                                     // DIAMETER_EQUAL_AREA
            o[13] = dn / (double)((unsigned long long)w * h);                 // EXTENT
            o[14] = (double)w / (double)h;                                    // ASPECT_RATIO
        }
    }
    // ---- convex hull (convex_hull_nontriv.cpp:68-120): the monotone chain over the column extremes --------------------------------
    if (do_hull && n >= 2) {
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
        {
            const int nu = S.n_up, nl = S.n_lo;
            for (int j = tid; j < nl; j += kMB) {
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
            S.n_hull = nh;
        }
        __syncthreads();
        // polygon_area's sum and hull_boundary_points over the closed vertex cycle: integers, any order
        {
            const int nh = S.n_hull;
            long long a2 = 0;
            unsigned long long bp = 0;
            for (int i = tid; i < nh; i += kMB) {
                const uint32_t p = up[i], q = up[i + 1 < nh ? i + 1 : 0];
                const long long x1 = p & 0xFFFFu, y1 = p >> 16, x2 = q & 0xFFFFu, y2 = q >> 16;
                a2 += x1 * y2 - y1 * x2;
                if (nh >= 2) bp += gcd_u32((uint32_t)(x2 > x1 ? x2 - x1 : x1 - x2), (uint32_t)(y2 > y1 ? y2 - y1 : y1 - y2));
            }
            unsigned long long ua = wave_add((unsigned long long)a2);
            bp = wave_add(bp);
            if (lane == 0) { atomicAdd(&S.twoA, ua); atomicAdd(&S.B, bp); }
        }
        __syncthreads();
    }
    // ---- perimeter (contour.cpp:960-974): wave 0, the terms in the reference's order ---------------------------------------------
    if ((do_con || do_hull) && tid < 64) {
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
            for (int t = 0; t < cnt; t++) per += __shfl(term, t, 64);         // one dependent add per point
        }
        if (lane == 0) S.per = per;
    }
    __syncthreads();
    const double per = S.per;
    if (do_hull && tid == 0) {
        const long long a2 = (long long)S.twoA;
        const unsigned long long twice = (unsigned long long)(a2 < 0 ? -a2 : a2) + S.B;   // 2 |A| + B
        const double area = (double)twice / 2.0 + 1.0;
        double* const o = row_out + R.col_hull;
        o[0] = sqrt(4.0 * kPi * (double)n / (per * per));                     // CIRCULARITY (+inf without a contour)
        o[1] = area;
        o[2] = (double)n / area;
    }
    // ---- contour columns (contour.cpp:935-986) --------------------------------------------------------------------------------
    if (!do_con)
        return;
    double* const o = row_out + R.col_contour;
    if (nK == 0) {
        if (tid < kMorphContourCols) o[tid] = 0.0;
        return;
    }
    {
        unsigned long long es = 0;
        uint32_t e0 = 0xFFFFFFFFu, e1 = 0u;
        bool outside = false;
        for (int i = tid; i < nK; i += kMB) {
            const uint32_t p = K[i], kx = p & 0xFFFFu, ky = p >> 16;          // padded coordinates: the pixel is (kx - 1, ky - 1)
            if (kx < 1u || ky < 1u || kx > w || ky > h) { outside = true; continue; }
            const uint32_t v = plane[(size_t)(ky - 1u) * w + (kx - 1u)];
            es += v; e0 = v < e0 ? v : e0; e1 = v > e1 ? v : e1;
        }
        if (__any(outside) && lane == 0) atomicCAS(R.status, 0, NYXHIP_ERR_INTERNAL);
        es = wave_add(es); e0 = wave_min(e0); e1 = wave_max(e1);
        if (lane == 0) { atomicAdd(&S.eS, es); atomicMin(&S.eMin, e0); atomicMax(&S.eMax, e1); }
    }
    __syncthreads();
    const double cnt = (double)nK, emean = (double)S.eS / cnt;
    double part = 0.0;
    for (int i = tid; i < nK; i += kMB) {
        const uint32_t p = K[i], kx = p & 0xFFFFu, ky = p >> 16;
        if (kx < 1u || ky < 1u || kx > w || ky > h) continue;
        const double e = (double)plane[(size_t)(ky - 1u) * w + (kx - 1u)] - emean;
        part += e * e;
    }
    const double em2 = block_sum(part, S, tid);
    if (tid == 0) {
        o[0] = per;
        o[1] = per / kPi;                                                     // DIAMETER_EQUAL_PERIMETER
        o[2] = emean;
        o[3] = nK > 2 ? sqrt(em2 / (double)(nK - 1)) : 0.0;                   // Moments4::std (moments.h:80)
        o[4] = (double)S.eMax;
        o[5] = (double)S.eMin;
        o[6] = (double)S.eS;
    }
}

} // namespace

__global__ __launch_bounds__(kMB) void roi_morph_kernel(const MorphArgs R)
{
    __shared__ MorphShared S;
    extern __shared__ __attribute__((aligned(16))) unsigned char morph_lds[];  // [kMorphBytesPerCol * cols_cap] tables | u32[plane_cap]
    const int tid = threadIdx.x;
    const uint64_t roi = R.roi_index ? R.roi_index[blockIdx.x] : blockIdx.x;
    if (roi >= R.n_roi)
        return;
    const uint64_t off = R.px_offset[roi];
    const uint32_t n = (uint32_t)(R.px_offset[roi + 1] - off);
    const uint32_t w = R.bbox_w[roi], h = R.bbox_h[roi];
    double* const row_out = R.out + roi * R.ld;
    const int n_cols = morph_n_columns(R.morph);
    const bool need_tab = (R.morph & NYXHIP_MORPH_HULL) != 0, need_plane = (R.morph & NYXHIP_MORPH_CONTOUR) != 0;
    const uint64_t cells = (uint64_t)w * h;
    const bool big = (need_tab && w > R.cols_cap) || (need_plane && cells > R.plane_cap);
    if (big) {
        if (R.defer_big)
            return;                                                          // served by the launch over the list of such ROIs
        if (!R.ws || (need_tab && w > R.ws_cols) || (need_plane && cells > R.ws_cells)) {   // (a box beyond what the caller stated)
            if (tid == 0) atomicCAS(R.status, 0, NYXHIP_ERR_ROI_TOO_LARGE);
            for (int c = tid; c < n_cols; c += kMB) row_out[c] = __longlong_as_double(0x7ff8000000000000LL);
            return;
        }
    }
    if (n == 0 || w == 0 || h == 0) {                                        // a blank ROI: zeros
        for (int c = tid; c < n_cols; c += kMB) row_out[c] = 0.0;
        return;
    }
    const unsigned long long ox = R.origin_x ? R.origin_x[roi] : 0u, oy = R.origin_y ? R.origin_y[roi] : 0u;
    const bool reads_contour = (R.morph & (NYXHIP_MORPH_CONTOUR | NYXHIP_MORPH_HULL)) != 0;
    const uint32_t* const K = reads_contour ? R.ws_contour + off : nullptr;
    const int nK = reads_contour ? (int)R.n_contour[roi] : 0;
    if (big) {
        unsigned char* const blk = R.ws + (uint64_t)blockIdx.x * R.ws_stride;
        morph_body(R, S, blk, R.ws_cols, (uint32_t*)(blk + (((uint64_t)kMorphBytesPerCol * R.ws_cols + 255) & ~255ull)), off, n, w, h, ox, oy, K, nK,
                   row_out, tid);
    } else
        morph_body(R, S, morph_lds, R.cols_cap, (uint32_t*)(morph_lds + (size_t)kMorphBytesPerCol * R.cols_cap), off, n, w, h, ox, oy, K, nK,
                   row_out, tid);
}

__device__ bool MorphBig::operator()(uint64_t i, uint32_t* hdr) const
{
    const uint32_t w = bw[i], h = bh[i];
    const uint64_t c = (uint64_t)w * h;
    if (w <= cols && c <= cells)
        return false;
    atomicMax(&hdr[1], w);
    atomicMax(&hdr[2], (uint32_t)(c > 0xFFFFFFFFull ? 0xFFFFFFFFull : c));
    return true;
}
template int deferred_classify<MorphBig>(uint64_t, const MorphBig&, uint32_t*, hipStream_t);

int launch_roi_morph(const MorphArgs& a, void* stream, uint32_t grid)
{
    if (grid == 0)
        return 0;
    const uint32_t dyn = kMorphBytesPerCol * a.cols_cap + 4u * a.plane_cap;   // (<= 24 KiB + 32 KiB)
    hipLaunchKernelGGL(roi_morph_kernel, dim3(grid), dim3(kMB), dyn, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace nyxhip
