// roi_vol.hip -- volumes (3-D): the voxel-intensity block and the 3-D GLCM block of the reference's Feature3D enum (gfx950).
//
//   vol_bin_kernel        the binned box of every ROI of a chunk -- one byte per cell, the level of features/texture_feature.h:52-76
//                         (bin_pixel of device_math.h, the code the 2-D texture kernels follow), the background level outside the
//                         cloud (the caller fills the boxes with it) -- scattered from the voxel cloud into the global workspace
//   vol_glcm_kernel       one workgroup per (ROI, direction of shifts[], 3d_glcm.cpp:16-31): the levels that occur (a 128-bit presence
//                         map: the sorted unique levels of radiomics binning, the largest level of IBSI mode, :285-317), the pair sweep
//                         over the box with integer LDS atomics into the Ng x Ng uint32 matrix (:326-371), and the 30 columns of the
//                         direction through the closing routine the 2-D kernels use (glcm_rows.h; 3d_glcm.cpp:438-1077 agrees with
//                         glcm.cpp term by term except for the two guards named at the call).  A box of at most kVolLdsCells cells is
//                         staged in LDS first; a larger one is read where it lies.
//   vol_glcm_ave_kernel   the 29 _AVE columns: a lane per (ROI, code), the 13 directional values in the order of std::reduce
//   vol_intensity_kernel  one workgroup per ROI: the voxel values, as offsets from the minimum, sorted in the global workspace (a stable
//                         4-bit LSD radix sort over the bits the range has), then intensity_from_table (intensity_table.h) over the
//                         sorted array as its table -- every closing formula is the 2-D one (3d_intensity.cpp:45-183 against
//                         intensity.cpp:57-192: the same text but for COVERED_IMAGE_INTENSITY_RANGE without a slide, which is 1 here)
//
// Everything that more than one thread adds to is an integer (LDS atomics); every floating-point sum runs in a fixed order.  Nothing of
// an ROI's row depends on another ROI: each workgroup reads its own ROI, its own box and the launch-wide settings only.
// Built with -ffp-contract=off (device_math.h).
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_kernel.h"
#include "launch_util.h"
#include "glcm_rows.h"
#include "intensity_table.h"
#include "roi_vol.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

// shifts[] of 3d_glcm.cpp:16-31: (dx, dy, dz)
__constant__ int c_vol_shift[kVolDirs][3] = {{1, 1, 1}, {1, 1, 0}, {1, 1, -1}, {1, 0, 1}, {1, 0, 0}, {1, 0, -1}, {1, -1, 1},
                                             {1, -1, 0}, {1, -1, -1}, {0, 1, 1}, {0, 1, 0}, {0, 1, -1}, {0, 0, 1}};

struct VolRoi {
    uint64_t roi, off, n64;
    uint32_t w, h, d, vmin, vmax;
    uint64_t cells;
};
__device__ __forceinline__ VolRoi vol_roi(const VolArgs& A, uint32_t j)
{
    VolRoi R;
    R.roi = A.roi0 + j;
    R.off = A.px_offset[R.roi];
    R.n64 = A.px_offset[R.roi + 1] - R.off;
    R.w = R.h = R.d = 1u;                                  // (the intensity block alone comes without boxes)
    if (A.bbox_w) { R.w = A.bbox_w[R.roi]; R.h = A.bbox_h[R.roi]; R.d = A.bbox_d[R.roi]; }
    R.vmin = A.vmin[R.roi]; R.vmax = A.vmax[R.roi];
    const bool sides = R.w <= kVolMaxSide && R.h <= kVolMaxSide && R.d <= kVolMaxSide;
    R.cells = sides ? (uint64_t)R.w * R.h * R.d : ~0ull;
    return R;
}
// what no kernel of the unit touches (vol_bin_kernel / vol_intensity_kernel raise the status): beyond what the strides were sized for
__device__ __forceinline__ bool vol_box_fits(const VolArgs& A, const VolRoi& R) { return R.cells <= (uint64_t)A.max_cells && R.cells <= (uint64_t)kVolMaxCells; }
__device__ __forceinline__ bool vol_levels_fit(const VolArgs& A, const VolRoi& R) { return A.grey_info != 0 || R.vmax <= kVolLevelCap; }

__global__ __launch_bounds__(256) void vol_bin_kernel(const VolArgs A)
{
    const int tid = threadIdx.x;
    const VolRoi R = vol_roi(A, blockIdx.y);
    if (R.n64 == 0) return;
    const bool first = tid == 0 && blockIdx.x == 0;
    if (R.cells == 0) { if (first) atomicCAS(A.status, 0, NYXHIP_ERR_INVALID_ARG); return; }   // voxels, and no box to hold them
    if (!vol_box_fits(A, R)) { if (first) atomicCAS(A.status, 0, NYXHIP_ERR_ROI_TOO_LARGE); return; }
    if (!vol_levels_fit(A, R)) { if (first) atomicCAS(A.status, 0, NYXHIP_ERR_UNSUPPORTED); return; }
    unsigned char* const box = A.boxes + (uint64_t)blockIdx.y * A.box_stride;
    const int g = A.grey_info;
    // a flat ROI under radiomics binning divides by a zero bin width in the reference (texture_feature.h:110-111, NaN to integer:
    // undefined); here every voxel of such an ROI has level 0, so every direction is blank
    const bool flat = g < 0 && R.vmax == R.vmin;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + (uint64_t)tid; i < R.n64; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t x = A.x[R.off + i], y = A.y[R.off + i], z = A.z[R.off + i];
        if (x >= R.w || y >= R.h || z >= R.d) { atomicCAS(A.status, 0, NYXHIP_ERR_INVALID_ARG); continue; }   // never stored
        uint32_t lvl = flat ? 0u : bin_pixel(A.inten[R.off + i], R.vmin, R.vmax, g);
        if (lvl > kVolLevelCap) { atomicCAS(A.status, 0, NYXHIP_ERR_UNSUPPORTED); lvl = 0; }                  // an intensity above the stated maximum (IBSI mode)
        box[((uint32_t)z * R.h + y) * R.w + x] = (unsigned char)lvl;
    }
}

// LDS of vol_glcm_kernel for a matrix order ng and a staging area of stage_cells bytes (16-aligned)
__host__ __device__ inline uint32_t vol_glcm_lds_mat(uint32_t ng) { return (4u * ng * ng + 15u) & ~15u; }
__host__ __device__ inline uint32_t vol_glcm_lds(uint32_t ng, uint32_t stage_cells) { return vol_glcm_lds_mat(ng) + 8u * (6u * ng + 32u) + 256u + stage_cells; }

__global__ __launch_bounds__(256) void vol_glcm_kernel(const VolArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ unsigned long long s_pres[2];
    __shared__ uint32_t s_total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dir = blockIdx.x;
    const VolRoi R = vol_roi(A, blockIdx.y);
    double* const orow = A.out + R.roi * A.ld + A.col_glcm;
    if (R.n64 == 0 || R.cells == 0) {                      // no voxels: the direction's 30 values are soft_nan
        if (tid < kVolGlcmAngled) orow[tid * kVolDirs + dir] = A.soft_nan;
        return;
    }
    if (!vol_box_fits(A, R) || !vol_levels_fit(A, R)) return;   // (vol_bin_kernel raised the status)
    const int g = A.grey_info;
    const uint32_t ngb = A.ng_bound;
    uint32_t* const P = (uint32_t*)lds_raw;                                     // [Ng x Ng] centre level x neighbour level
    double* const Iv = (double*)(lds_raw + vol_glcm_lds_mat(ngb));             // [ngb] level values I[] (3d_glcm.cpp:285-317)
    double* const scr = Iv + ngb;                                               // [5 ngb] marginals of the closing routine
    double* const f = scr + 5 * ngb;                                            // [32] the direction's values, 2-D slot order
    unsigned char* const lmap = (unsigned char*)(f + 32);                       // [256] level -> matrix index
    unsigned char* const stage = lmap + 256;                                    // [stage_cells] the binned box, when it fits
    const unsigned char* const box = A.boxes + (uint64_t)blockIdx.y * A.box_stride;
    const uint32_t cells = (uint32_t)R.cells;
    const bool staged = cells <= kVolLdsCells;
    if (tid < 2) s_pres[tid] = 0ull;
    if (tid == 0) s_total = 0u;
    __syncthreads();
    // ---- which levels occur (bit l - 1 = level l), and the copy into LDS.  The box is read a word at a time: its stride is a multiple of
    // 256 bytes and the bytes behind the last cell hold the background level, which adds nothing a cell outside the cloud does not add
    {
        unsigned long long lo = 0ull, hi = 0ull;
        const uint32_t* const bw = (const uint32_t*)box;
        const uint32_t nwords = (cells + 3u) >> 2;
        for (uint32_t i = tid; i < nwords; i += 256u) {
            const uint32_t v = bw[i];
            if (staged) ((uint32_t*)stage)[i] = v;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t l = (v >> (8 * k)) & 255u;
                if (l) {
                    const uint32_t bit = l - 1u;
                    if (bit < 64u) lo |= 1ull << bit; else hi |= 1ull << (bit & 63u);
                }
            }
        }
        if (lo) atomicOr(&s_pres[0], lo);
        if (hi) atomicOr(&s_pres[1], hi);
    }
    __syncthreads();
    const unsigned long long plo = s_pres[0], phi = s_pres[1];
    // matrix order: matlab binning: the level count; IBSI: the largest level that occurs (:309-316); radiomics: the distinct levels (:288-294)
    const int Ng = g > 0 ? g : g == 0 ? (phi ? 128 - __clzll((long long)phi) : plo ? 64 - __clzll((long long)plo) : 0) : __popcll(plo) + __popcll(phi);
    if (Ng == 0 || (uint32_t)Ng > ngb) {                   // no level above 0 anywhere: blank (the second test cannot hold: the host sized ngb)
        if (tid < kVolGlcmAngled) orow[tid * kVolDirs + dir] = A.soft_nan;
        return;
    }
    if (tid < 128) {
        const uint32_t l = (uint32_t)tid + 1u;
        if (g < 0) {
            const bool here = tid < 64 ? (plo >> tid) & 1ull : (phi >> (tid - 64)) & 1ull;
            const int rank = tid < 64 ? __popcll(plo & ((1ull << tid) - 1ull)) : __popcll(plo) + __popcll(phi & ((1ull << (tid - 64)) - 1ull));
            if (here) { lmap[l] = (unsigned char)rank; Iv[rank] = (double)l; }
        } else if (tid < Ng) {
            lmap[l] = (unsigned char)tid; Iv[tid] = (double)l;
        }
    }
    for (int i = tid; i < Ng * Ng; i += 256) P[i] = 0u;
    __syncthreads();
    // ---- the pair sweep (3d_glcm.cpp:326-371): centre b = D(z, y, x), neighbour a = D(z + dz, y + dy, x + dx) where the neighbour lies in
    // the box (both borders: dy and dz may be negative; dx is never); a pair with a zero level is skipped (no level is 0 under matlab
    // binning); GLCM.xy(a, b)++ = P[b * Ng + a], and the mirrored cell when the count is symmetric.  A row of the box is shared by LW
    // lanes, LW the power of two that covers min(w, 64): one division per row.
    {
        const int dx = c_vol_shift[dir][0] * A.offset, dy = c_vol_shift[dir][1] * A.offset, dz = c_vol_shift[dir][2] * A.offset;
        const unsigned char* const D = staged ? (const unsigned char*)stage : box;
        const bool sym = A.symmetric != 0 || g <= 0;
        uint32_t lw_log = 6;
        while (lw_log > 3 && (1u << (lw_log - 1)) >= R.w) lw_log--;
        const uint32_t LW = 1u << lw_log, rpw = 64u >> lw_log, sub = (uint32_t)lane >> lw_log, l = (uint32_t)lane & (LW - 1u);
        const uint32_t rows = R.h * R.d;
        uint32_t cnt = 0;
        for (uint32_t rr = (uint32_t)wave * rpw + sub; rr < rows; rr += 4u * rpw) {
            const uint32_t z = rr / R.h, y = rr - z * R.h;
            const long long nz = (long long)z + dz, ny = (long long)y + dy;
            if (nz < 0 || nz >= (long long)R.d || ny < 0 || ny >= (long long)R.h) continue;
            const uint32_t base = rr * R.w, nbase = ((uint32_t)nz * R.h + (uint32_t)ny) * R.w;
            for (uint64_t x = l; x + (uint64_t)dx < (uint64_t)R.w; x += LW) {
                const uint32_t b = D[base + (uint32_t)x], a = D[nbase + (uint32_t)x + (uint32_t)dx];
                if (a == 0u || b == 0u) continue;
                const uint32_t ia = lmap[a], ib = lmap[b];
                atomicAdd(&P[ib * (uint32_t)Ng + ia], 1u);
                if (sym) atomicAdd(&P[ia * (uint32_t)Ng + ib], 1u);
                cnt++;
            }
        }
        if (cnt) atomicAdd(&s_total, cnt);
    }
    __syncthreads();
    if (s_total == 0u) {                                   // blank matrix: 30 x soft_nan (3d_glcm.cpp:184-218)
        if (tid < kVolGlcmAngled) orow[tid * kVolDirs + dir] = A.soft_nan;
        return;
    }
    if (wave == 0) {
        // The closing formulas of 3d_glcm.cpp:438-1077 are those of glcm.cpp but for two guards the 2-D class has and the 3-D class lacks:
        // f_corr returns tmp1 / (sr * sc) as it comes (0 / 0 = NaN where a marginal has no variance) and f_info_meas_corr1 returns
        // (HXY - HXY1) / HX as it comes (0 / 0 = NaN for a single level).  The shared routine writes its `soft_nan` argument in exactly
        // those two cases, so it is handed NaN; the blank matrix, its other use of the argument, was answered above.
        glcm_features_rows<false, 64, 3>(P, 1, Ng, Iv, scr, 5 * Ng, __builtin_nan(""), f, lane);
        // Feature3D order: GLCM_ACOR, GLCM_ASM, then as the 2-D enum (featureset.h:739-768)
        if (lane < kVolGlcmAngled) orow[lane * kVolDirs + dir] = f[lane == 0 ? G_ACOR : lane == 1 ? G_ASM : lane];
    }
}

// calc_ave (texture_feature.h:121-130): std::reduce(begin, end) / 13.  libstdc++'s std::reduce over random-access iterators takes the
// values four at a time -- init = init + ((v0 + v1) + (v2 + v3)) -- and the rest one by one; that order is kept.
__global__ __launch_bounds__(256) void vol_glcm_ave_kernel(const VolArgs A)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= A.n_roi * (uint64_t)kVolGlcmAve) return;
    const uint32_t j = (uint32_t)(t / kVolGlcmAve), k = (uint32_t)(t - (uint64_t)j * kVolGlcmAve);
    const VolRoi R = vol_roi(A, j);
    double* const orow = A.out + R.roi * A.ld + A.col_glcm;
    if (R.n64 == 0 || R.cells == 0) { orow[kVolGlcmAngled * kVolDirs + k] = A.soft_nan; return; }
    if (!vol_box_fits(A, R) || !vol_levels_fit(A, R)) return;
    const int c2 = c_glcm_ave_order[k];                    // the _AVE codes of Feature3D follow the 2-D order (featureset.h:769-797)
    const double* const v = orow + (c2 == G_ASM ? 1 : c2 == G_ACOR ? 0 : c2) * kVolDirs;
    double init = 0.0;
    init = init + ((v[0] + v[1]) + (v[2] + v[3]));
    init = init + ((v[4] + v[5]) + (v[6] + v[7]));
    init = init + ((v[8] + v[9]) + (v[10] + v[11]));
    init = init + v[12];
    orow[kVolGlcmAngled * kVolDirs + k] = init / 13.0;
}

// ---- intensity: the sorted offsets of an ROI as the table of intensity_from_table -------------------------------------------------
// entry i = the i-th smallest voxel; cum(i) = i + 1 holds for the routine's uses (order statistics, counts below a bound, counts inside
// a range) because first_ge returns the FIRST entry of a run of equal values
struct VolSortedTab {
    const uint32_t* S; uint32_t m;
    __device__ __forceinline__ uint32_t off(uint32_t i) const { return S[i]; }
    __device__ __forceinline__ uint32_t cum(uint32_t i) const { return i + 1u; }
    __device__ __forceinline__ uint32_t first_ge(uint64_t d) const
    {
        if (d > 0xFFFFFFFFull) return m;
        uint32_t lo = 0, hi = m;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (S[mid] < (uint32_t)d) lo = mid + 1u; else hi = mid;
        }
        return lo;
    }
};
// the sums over the voxels' own values (offsets from the minimum, sorted)
struct VolSortedSums {
    const uint32_t* S; uint32_t n, vmin;
    __device__ __forceinline__ void central(double mean, bool blank, double (&acc)[6], uint32_t& mode_off, const IntensityScratch& T, int tid) const
    {
        const int lane = tid & 63, wave = tid >> 6;
        const double meanx = mean - (double)vmin;
        uint32_t best_c = 0, best_i = 0;
        for (uint32_t i = tid; i < n; i += 256u) {
            const uint32_t x = S[i];
            if (!blank) {
                const double d = (double)x - meanx, d2 = d * d;
                acc[0] += fabs(d);
                acc[1] += d2;
                acc[2] += d2 * d;
                acc[3] += d2 * d2;
                acc[4] += d2 * d2 * d;
                acc[5] += d2 * d2 * d2;
            }
            // mode (histogram.h:289-309): the longest run, the smallest value on ties.  A run is measured where it starts: a gallop, then a
            // binary search for its end
            if (i == 0 || S[i - 1] != x) {
                uint32_t len = 1;
                if (i + 1u < n && S[i + 1u] == x) {
                    uint64_t step = 2;
                    while ((uint64_t)i + step < n && S[i + step] == x) step <<= 1;
                    uint64_t lo = (uint64_t)i + (step >> 1), hi = (uint64_t)i + step < n ? (uint64_t)i + step : n;   // S[lo] == x, S[hi] != x (or hi == n)
                    while (hi - lo > 1) {
                        const uint64_t mid = lo + ((hi - lo) >> 1);
                        if (S[mid] == x) lo = mid; else hi = mid;
                    }
                    len = (uint32_t)(hi - i);
                }
                if (len > best_c) { best_c = len; best_i = i; }            // (i ascends: the first of equal runs is the smallest value)
            }
        }
        const uint32_t mc_w = wave_max_u32(best_c);
        const uint32_t cand = best_c == mc_w ? best_i : 0xFFFFFFFFu;
        const uint32_t bi_w = ~wave_max_u32(~cand);
        __syncthreads();
        if (lane == 0) { T.w[4 + wave] = mc_w; T.w[8 + wave] = bi_w; }
        __syncthreads();
        uint32_t mc = 0, mi = 0;
        for (int wv = 0; wv < 4; wv++) {
            const uint32_t c = T.w[4 + wv], i = T.w[8 + wv];
            if (c > mc || (c == mc && i < mi)) { mc = c; mi = i; }
        }
        mode_off = S[mi < n ? mi : 0u];
    }
    __device__ __forceinline__ void robust(uint32_t lo_off, uint32_t hi_off, bool some, double median, unsigned long long& sx, double& medad, int tid) const
    {
        const double medx = median - (double)vmin;
        for (uint32_t i = tid; i < n; i += 256u) {
            const uint32_t x = S[i];
            if (some && x >= lo_off && x <= hi_off) sx += (unsigned long long)vmin + x;
            medad += fabs((double)x - medx);
        }
    }
    __device__ __forceinline__ void spread(uint32_t lo_off, uint32_t hi_off, double mean1090, double& ad, int tid) const
    {
        const double mx = mean1090 - (double)vmin;
        for (uint32_t i = tid; i < n; i += 256u) {
            const uint32_t x = S[i];
            if (x >= lo_off && x <= hi_off) ad += fabs((double)x - mx);
        }
    }
};

__global__ __launch_bounds__(256) void vol_intensity_kernel(const VolArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];     // [104] + [n_hist + 8] words: the histogram bounds
    __shared__ uint32_t s_cnt[16 * 256];                                        // radix pass: [digit][thread]
    __shared__ double s_x[32];
    __shared__ unsigned long long s_u[8];
    __shared__ double s_stat[8];
    __shared__ double s_pq[8];
    __shared__ uint32_t s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const VolRoi R = vol_roi(A, blockIdx.x);
    double* const o = A.out + R.roi * A.ld + A.col_intensity;
    if (R.n64 == 0) {                                      // no voxels: the row is soft_nan
        for (int c = tid; c < kVolIntensityCols; c += 256) o[c] = A.soft_nan;
        return;
    }
    if (R.n64 > (uint64_t)A.max_px || R.vmax < R.vmin) {
        if (tid == 0) atomicCAS(A.status, 0, R.vmax < R.vmin ? NYXHIP_ERR_INVALID_ARG : NYXHIP_ERR_ROI_TOO_LARGE);
        return;
    }
    for (int c = tid; c < kVolIntensityCols; c += 256) o[c] = 0.0;               // what the class skips stays 0 (its members default to 0)
    const uint32_t n = (uint32_t)R.n64, vmin = R.vmin, range = R.vmax - R.vmin;
    uint32_t* src = A.keys + 2ull * blockIdx.x * A.key_stride;
    uint32_t* dst = src + A.key_stride;
    // ---- load: the two exact sums, the offsets from the minimum
    unsigned long long sum = 0, sumsq = 0;
    bool outside = false;
    const uint32_t* const gv = A.inten + R.off;
    for (uint32_t i = tid; i < n; i += 256u) {
        const uint32_t v = gv[i];
        sum += v;
        sumsq += (uint32_t)(v * v);                        // unsigned-int product, wraps (3d_intensity.cpp:79)
        outside |= v < vmin || v > R.vmax;
        src[i] = v - vmin;
    }
    if (outside) atomicCAS(A.status, 0, NYXHIP_ERR_INVALID_ARG);                 // min_inten / max_inten are not the cloud's extrema
    sum = wg4_sum_u64(sum, s_u, tid);
    __syncthreads();
    sumsq = wg4_sum_u64(sumsq, s_u, tid);
    if (__syncthreads_or(outside ? 1 : 0)) return;
    // ---- stable LSD radix sort, four bits a pass, over the bits the range has.  Thread t owns the keys [c0, c1) of every pass: it counts
    // its digits into its own sixteen counters, the 4096 counters are scanned in (digit, thread) order, and it places its keys in order
    const uint32_t cs = (n + 255u) / 256u;
    const uint32_t c0 = (uint64_t)tid * cs < n ? (uint32_t)tid * cs : n, c1 = (uint64_t)c0 + cs < n ? c0 + cs : n;
    const int bits = range ? 32 - __clz((int)range) : 0;
    for (int shift = 0; shift < bits; shift += 4) {
#pragma unroll
        for (int dg = 0; dg < 16; dg++) s_cnt[dg * 256 + tid] = 0u;
        for (uint32_t i = c0; i < c1; i++) s_cnt[((src[i] >> shift) & 15u) * 256u + (uint32_t)tid]++;
        __syncthreads();
        {
            uint32_t v[16], tot = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) { v[k] = s_cnt[16 * tid + k]; tot += v[k]; }
            const uint32_t sc = wave_scan_u32(tot);
            if (lane == 63) s_w[wave] = sc;
            __syncthreads();
            uint32_t run = sc - tot;
            for (int wv = 0; wv < wave; wv++) run += s_w[wv];
#pragma unroll
            for (int k = 0; k < 16; k++) { s_cnt[16 * tid + k] = run; run += v[k]; }
        }
        __syncthreads();
        for (uint32_t i = c0; i < c1; i++) {
            const uint32_t key = src[i];
            dst[s_cnt[((key >> shift) & 15u) * 256u + (uint32_t)tid]++] = key;
        }
        __syncthreads();
        uint32_t* const t = src; src = dst; dst = t;
    }
    __syncthreads();
    IntensityScratch T{s_x, s_u, s_stat, s_pq, s_w, (uint32_t*)lds_raw, (uint32_t*)lds_raw + 104};
    const bool have_slide = A.slide_min && A.slide_max;
    const double slide_range = have_slide ? A.slide_max[R.roi] - A.slide_min[R.roi] : 0.0;
    const VolSortedTab tab{src, n};
    const VolSortedSums ks{src, n, vmin};
    intensity_from_table(tab, ks, n, vmin, R.vmax, (double)sum, (double)sumsq, have_slide, slide_range, A.n_hist, o, T, tid);
    if (tid == 0 && !have_slide) o[I_COVERED_IMAGE_INTENSITY_RANGE] = 1.0;       // 3d_intensity.cpp:64-65 (the 2-D class leaves 0)
}

} // namespace

int vol_background_level(int grey_info) { return grey_info > 0 ? 1 : 0; }        // bin_array_matlab(0) = 1 (texture_feature.h:152-154)

int launch_vol_bin(const VolArgs& a, void* stream)
{
    if (a.n_roi == 0) return 0;
    uint32_t gx = (a.max_px + 2047u) / 2048u;
    gx = gx < 1u ? 1u : gx > 256u ? 256u : gx;
    hipLaunchKernelGGL(vol_bin_kernel, dim3(gx, (uint32_t)a.n_roi), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_vol_glcm(const VolArgs& a, void* stream)
{
    if (a.n_roi == 0) return 0;
    static DeviceOnce optin;
    if (int orc = optin.run([]() -> int {
            return (int)hipFuncSetAttribute((const void*)vol_glcm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)vol_glcm_lds(kVolLevelCap, kVolLdsCells));
        }))
        return orc;
    hipLaunchKernelGGL(vol_glcm_kernel, dim3(kVolDirs, (uint32_t)a.n_roi), dim3(256), vol_glcm_lds(a.ng_bound, a.stage_cells), (hipStream_t)stream, a);
    if (int rc = (int)hipGetLastError()) return rc;
    const uint64_t t = a.n_roi * (uint64_t)kVolGlcmAve;
    hipLaunchKernelGGL(vol_glcm_ave_kernel, dim3((uint32_t)((t + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_vol_intensity(const VolArgs& a, void* stream)
{
    if (a.n_roi == 0) return 0;
    static DeviceOnce optin;
    if (int orc = optin.run([]() -> int {
            return (int)hipFuncSetAttribute((const void*)vol_intensity_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (112 + 16384 + 8));
        }))
        return orc;
    hipLaunchKernelGGL(vol_intensity_kernel, dim3((uint32_t)a.n_roi), dim3(256), 4u * (112u + a.n_hist + 8u), (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace nyxhip
