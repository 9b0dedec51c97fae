// roi_chords.hip -- ChordsFeature of the shape block (features/chords.cpp:11-111 of the reference): MAXCHORDS_* and ALLCHORDS_*,
// on Rotation::rotate_cloud (rotation.cpp:70-91), ImageMatrix(cloud) (image_matrix.h:256-277), ImageMatrix::get_chlen
// (image_matrix.cpp:206-237), Moments2 (moments.h:10-45) and TrivialHistogram (histogram.h:115-119, :268-309).
//
//   roi_chords_kernel   One 256-thread workgroup per ROI over the pixel cloud; 20 angles one after the other.
//                       Bounds    every thread turns its pixels about the centre of the absolute box in fp64 (sin / cos from the
//                                 host, in the kernel arguments), rounds to float, truncates toward zero: the tight box of the
//                                 turned cloud (integer min / max through the waves).
//                       Plane     one BIT per cell, column-major, every column padded to whole words: LDS atomic OR.  An ROI with
//                                 zero-intensity pixels resolves "the last pixel of the cloud decides the cell" first: a word per
//                                 cell, atomic max over 2 * (index + 1) + (intensity != 0), whose low bit then goes to the bit plane.
//                                 (Global planes: blk_sync<true> at the exchange points, as in the other workspace kernels.)
//                       Columns   one lane per scanned column: the longest run of ones that a zero closes, by count-trailing-zeros
//                                 steps over the column's words (a run that reaches the last row is dropped, as in get_chlen).
//                                 The chords > 0 are appended to the ROI's list in column order (ballot ranks).
//                       Closing   lane 0 closes the <= 20 per-angle maxima, a lane of another wave the <= 3980 chords: Welford's
//                                 mean / M2 in insertion order, the reference's own sequence of fp64 operations.  Median and mode of
//                                 the chords come from an LDS radix sort of the maxima AND the chords: the reference's histogram
//                                 object is not cleared between its two uses (histogram.h:115-119), so every maximum counts twice.
//   ROIs whose plane bound exceeds the LDS plane, and ROIs with zero-intensity pixels, are served by a launch over their list with
//   planes in global memory (ChordArgs::ws); the code is the same.
//   Every value is an integer, a table value or a fixed sequence of fp64 operations: a row depends neither on scheduling nor on the
//   path (LDS / HBM), and on the pixel order only where the reference does (zero-intensity pixels sharing a cell with others).
//   Built with -ffp-contract=off like every unit; no reciprocal forms.
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "sort_lds.h"
#include "roi_chords.h"
#include "launch_util.h"
#include "deferred_list.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

constexpr int kHB = 256;
constexpr int kHW = kHB / 64;

struct ChordShared {
    uint32_t U[kChordsMaxAll + kChordsAngles];     // all chords in insertion order (angle-major, then column); the maxima behind them for the sort
    uint32_t hist[kHW * 256 + kHW];                // radix_sort's tables
    long long red[kHW][4];                         // per wave: min x, max x, min y, max y of the turned pixels
    uint32_t start[kChordsAngles + 1];             // U[start[k] .. start[k + 1]): the chords of angle k
    uint32_t amax[kChordsAngles];                  // the longest chord of angle k
    uint32_t wcnt[kHW];
    uint32_t n_all, n_mc, kmin, range;
    unsigned long long mode_key;
};

// ImageMatrix::get_chlen over one column of the bit plane (h rows in (h + 31) / 32 words; the bits behind row h - 1 are zero)
__device__ __forceinline__ uint32_t column_chord(const uint32_t* col, uint32_t h)
{
    uint32_t best = 0, cur = 0;
    for (uint32_t r0 = 0; r0 < h; r0 += 32) {
        const uint32_t word = col[r0 >> 5];
        const uint32_t nb = h - r0 < 32u ? h - r0 : 32u;
        if (word == 0u) { best = cur > best ? cur : best; cur = 0; continue; }
        if (word == 0xFFFFFFFFu && nb == 32u) { cur += 32u; continue; }
        uint32_t pos = 0;
        while (pos < nb) {
            const uint32_t rest = word >> pos;
            if (rest & 1u) {
                uint32_t t = ~rest ? (uint32_t)__builtin_ctz(~rest) : 32u;   // the ones from `pos` on
                t = t < nb - pos ? t : nb - pos;
                cur += t; pos += t;
            } else {
                best = cur > best ? cur : best; cur = 0;                    // a zero cell closes the run
                if (rest == 0u) break;                                      // (rows [pos, nb) are zero; behind nb there are no rows)
                pos += (uint32_t)__builtin_ctz(rest);
            }
        }
    }
    return best;                                                            // (`cur`: a run that reaches the last row is not counted)
}

template <bool kGlobal>
__device__ __forceinline__ void chords_body(const ChordArgs& R, ChordShared& S, uint32_t* bits, uint64_t cap_words, uint32_t* last, uint64_t cap_cells,
                                            uint32_t* sort_b, const uint16_t* xs, const uint16_t* ys, const uint32_t* it, uint32_t n, uint32_t w,
                                            uint32_t h, uint32_t ox, uint32_t oy, double* o, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    // the centre of the absolute box (chords.cpp:14-15)
    const long long xmin = ox, ymin = oy;
    const double cx = (double)(xmin + (xmin + (long long)w - 1)) / 2.0, cy = (double)(ymin + (ymin + (long long)h - 1)) / 2.0;
    if (tid == 0) { S.n_all = 0; S.mode_key = 0ull; }
    __syncthreads();
    auto turned = [&](uint32_t i, double sn, double cs, long long& xi, long long& yi) {
        const double px = (double)((long long)xs[i] + xmin), py = (double)((long long)ys[i] + ymin);
        const double xr = (px - cx) * cs - (py - cy) * sn + cx;
        const double yr = (py - cy) * cs + (px - cx) * sn + cy;
        xi = (long long)(float)xr; yi = (long long)(float)yr;               // Pixel2(float, float, ...): truncation toward zero
    };
    for (int k = 0; k < kChordsAngles; k++) {
        const double sn = R.sn[k], cs = R.cs[k];
        // ---- the tight box of the turned cloud -----------------------------------------------------------------------------------
        long long x0 = 0x7fffffffffffffffLL, x1 = -x0, y0 = x0, y1 = -x0;
        for (uint32_t i = (uint32_t)tid; i < n; i += kHB) {
            long long xi, yi;
            turned(i, sn, cs, xi, yi);
            x0 = xi < x0 ? xi : x0; x1 = xi > x1 ? xi : x1; y0 = yi < y0 ? yi : y0; y1 = yi > y1 ? yi : y1;
        }
#pragma unroll
        for (int q = 32; q > 0; q >>= 1) {
            const long long a0 = __shfl_xor(x0, q, 64), a1 = __shfl_xor(x1, q, 64), b0 = __shfl_xor(y0, q, 64), b1 = __shfl_xor(y1, q, 64);
            x0 = a0 < x0 ? a0 : x0; x1 = a1 > x1 ? a1 : x1; y0 = b0 < y0 ? b0 : y0; y1 = b1 > y1 ? b1 : y1;
        }
        if (lane == 0) { S.red[wave][0] = x0; S.red[wave][1] = x1; S.red[wave][2] = y0; S.red[wave][3] = y1; }
        __syncthreads();
        x0 = S.red[0][0]; x1 = S.red[0][1]; y0 = S.red[0][2]; y1 = S.red[0][3];
#pragma unroll
        for (int q = 1; q < kHW; q++) {
            x0 = S.red[q][0] < x0 ? S.red[q][0] : x0; x1 = S.red[q][1] > x1 ? S.red[q][1] : x1;
            y0 = S.red[q][2] < y0 ? S.red[q][2] : y0; y1 = S.red[q][3] > y1 ? S.red[q][3] : y1;
        }
        const uint64_t W = (uint64_t)(x1 - x0) + 1, H = (uint64_t)(y1 - y0) + 1;
        const uint64_t wpc = (H + 31) / 32, words = W * wpc;
        if (W > 0xFFFFFFu || H > 0xFFFFFFu || words > cap_words || (last && W * H > cap_cells)) {
            // (beyond the bound of chords_plane_words: not reached by boxes that are what the batch states)
            if (tid == 0) {
                atomicCAS(R.status, 0, NYXHIP_ERR_ROI_TOO_LARGE);
                for (int i = 0; i < kChordsCols; i++) o[i] = __longlong_as_double(0x7ff8000000000000LL);
            }
            return;
        }
        // ---- the plane ---------------------------------------------------------------------------------------------------------------
        for (uint64_t i = (uint64_t)tid; i < words; i += kHB) bits[i] = 0u;
        if (last)
            for (uint64_t i = (uint64_t)tid; i < W * H; i += kHB) last[i] = 0u;
        blk_sync<kGlobal>();
        for (uint32_t i = (uint32_t)tid; i < n; i += kHB) {
            long long xi, yi;
            turned(i, sn, cs, xi, yi);
            const uint64_t c = (uint64_t)(xi - x0), r = (uint64_t)(yi - y0);
            if (last) atomicMax(&last[c * H + r], ((i + 1u) << 1) | (it[i] != 0u ? 1u : 0u));
            else atomicOr(&bits[c * wpc + (r >> 5)], 1u << (r & 31u));
        }
        blk_sync<kGlobal>();
        if (last) {
            for (uint64_t i = (uint64_t)tid; i < W * H; i += kHB) {
                if (last[i] & 1u) {
                    const uint64_t c = i / H, r = i - c * H;
                    atomicOr(&bits[c * wpc + (r >> 5)], 1u << (r & 31u));
                }
            }
            blk_sync<kGlobal>();
        }
        // ---- the columns (chords.cpp:37-47) --------------------------------------------------------------------------------------
        const uint32_t step = W >= 2u * kChordsSide ? (uint32_t)W / kChordsSide : 1u;
        const uint32_t nsel = ((uint32_t)W + step - 1u) / step;              // (<= kChordsMaxCols < kHB)
        uint32_t ch = 0;
        if ((uint32_t)tid < nsel) ch = column_chord(bits + (uint64_t)tid * step * wpc, (uint32_t)H);
        const unsigned long long bal = __ballot(ch > 0u);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        uint32_t mx = ch;
#pragma unroll
        for (int q = 32; q > 0; q >>= 1) { const uint32_t a = __shfl_xor(mx, q, 64); mx = a > mx ? a : mx; }
        if (lane == 0) { S.wcnt[wave] = (uint32_t)__popcll(bal); S.red[wave][0] = (long long)mx; }
        __syncthreads();
        {
            uint32_t base = S.n_all, total = 0, m = 0;
#pragma unroll
            for (int q = 0; q < kHW; q++) {
                if (q < wave) base += S.wcnt[q];
                total += S.wcnt[q];
                m = (uint32_t)S.red[q][0] > m ? (uint32_t)S.red[q][0] : m;
            }
            if (ch > 0u) S.U[base + rank] = ch;
            __syncthreads();
            if (tid == 0) { S.start[k] = S.n_all; S.amax[k] = m; S.n_all += total; S.start[k + 1] = S.n_all; }
        }
        __syncthreads();
    }
    // ---- closing -------------------------------------------------------------------------------------------------------------------
    const uint32_t n_all = S.n_all;
    if (n_all == 0) {                                                        // MC is empty: the members keep their initial zeros (chords.cpp:59-60)
        if (tid < kChordsCols) o[tid] = 0.0;
        return;
    }
    uint32_t* const mcv = S.hist;                                            // [20] maxima of the angles that had a chord | [20] their angles
    if (tid == 0) {
        // MAXCHORDS_*: Moments2 over the maxima in angle order; mode and median of <= 20 values on this lane
        uint32_t* const mca = mcv + kChordsAngles;
        int m = 0;
        for (int k = 0; k < kChordsAngles; k++)
            if (S.amax[k] > 0u) { mcv[m] = S.amax[k]; mca[m] = (uint32_t)k; m++; }
        double mean = 0.0, M2 = 0.0;
        int i_min = 0, i_max = 0;
        for (int i = 0; i < m; i++) {
            const double x = (double)mcv[i];
            const double delta = x - mean, delta_n = delta / (double)(i + 1), term1 = delta * delta_n * (double)i;
            mean = mean + delta_n;
            M2 += term1;
            if (mcv[i] < mcv[i_min]) i_min = i;
            if (mcv[i] > mcv[i_max]) i_max = i;
        }
        uint32_t mode = 0; int best = 0;
        for (int i = 0; i < m; i++) {
            int c = 0;
            for (int j = 0; j < m; j++) c += mcv[j] == mcv[i];
            if (c > best || (c == best && mcv[i] < mode)) { best = c; mode = mcv[i]; }
        }
        // median: the element(s) of rank m / 2 (and m / 2 - 1) -- by counting, the list stays in angle order
        auto kth = [&](int kk) {
            for (int i = 0; i < m; i++) {
                int lt = 0, le = 0;
                for (int j = 0; j < m; j++) { lt += mcv[j] < mcv[i]; le += mcv[j] <= mcv[i]; }
                if (lt <= kk && kk < le) return mcv[i];
            }
            return 0u;
        };
        const double med = (m & 1) ? (double)kth(m / 2) : (double)(kth(m / 2) + kth(m / 2 - 1)) / 2.0;
        o[0] = (double)mcv[i_max]; o[1] = R.ang[mca[i_max]]; o[2] = (double)mcv[i_min]; o[3] = R.ang[mca[i_min]];
        o[4] = med; o[5] = mean; o[6] = (double)mode; o[7] = m > 2 ? sqrt(M2 / (double)(m - 1)) : 0.0;
        S.n_mc = (uint32_t)m;
    }
    if (tid == 64) {
        // ALLCHORDS_*: Moments2 over every chord in insertion order
        double mean = 0.0, M2 = 0.0;
        uint32_t i_min = 0, i_max = 0, v_min = S.U[0], v_max = S.U[0];
        for (uint32_t i = 0; i < n_all; i++) {
            const uint32_t v = S.U[i];
            const double x = (double)v;
            const double delta = x - mean, delta_n = delta / (double)(i + 1u), term1 = delta * delta_n * (double)i;
            mean = mean + delta_n;
            M2 += term1;
            if (v < v_min) { v_min = v; i_min = i; }
            if (v > v_max) { v_max = v; i_max = i; }
        }
        int k_min = 0, k_max = 0;                                            // the angles whose spans of U hold the two elements
        for (int k = 0; k < kChordsAngles; k++) {
            if (S.start[k] <= i_min && i_min < S.start[k + 1]) k_min = k;
            if (S.start[k] <= i_max && i_max < S.start[k + 1]) k_max = k;
        }
        o[8] = (double)v_max; o[9] = R.ang[k_max]; o[10] = (double)v_min; o[11] = R.ang[k_min];
        o[13] = mean; o[15] = n_all > 2u ? sqrt(M2 / (double)(n_all - 1u)) : 0.0;
        S.kmin = v_min; S.range = v_max - v_min;
    }
    __syncthreads();
    // the histogram's second use holds the maxima and the chords (initialize_uniques appends): sort both
    const uint32_t n_mc = S.n_mc, n_u = n_all + n_mc;
    uint32_t keep = 0;
    if ((uint32_t)tid < n_mc) keep = mcv[tid];
    __syncthreads();                                                         // (mcv lies in the sort's tables)
    if ((uint32_t)tid < n_mc) S.U[n_all + (uint32_t)tid] = keep;
    __syncthreads();
    const uint32_t* const srt = radix_sort<false, kHW, uint32_t>(S.U, sort_b, S.hist, n_u, S.kmin, S.range, tid);
    __syncthreads();
    // mode: the smallest among the most frequent -- every run's first element looks up where its run ends
    for (uint32_t i = (uint32_t)tid; i < n_u; i += kHB) {
        const uint32_t v = srt[i];
        if (i > 0 && srt[i - 1] == v) continue;
        uint32_t lo = i, hi = n_u;                                           // first index in (i, n_u] whose value differs
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (srt[mid] == v) lo = mid; else hi = mid; }
        atomicMax(&S.mode_key, ((unsigned long long)(hi - i) << 32) | (unsigned long long)(0xFFFFFFFFu - v));
    }
    __syncthreads();
    if (tid == 0) {
        o[12] = (n_u & 1u) ? (double)srt[n_u / 2] : (double)(srt[n_u / 2] + srt[n_u / 2 - 1]) / 2.0;
        o[14] = (double)(0xFFFFFFFFu - (uint32_t)(S.mode_key & 0xFFFFFFFFull));
    }
}

} // namespace

__host__ __device__ inline bool chords_listed(uint32_t w, uint32_t h, uint32_t min_inten, uint32_t lds_words)
{
    return min_inten == 0u || chords_plane_words(w, h) > (uint64_t)lds_words;
}

__global__ __launch_bounds__(kHB) void roi_chords_kernel(const ChordArgs R)
{
    __shared__ ChordShared S;
    extern __shared__ __attribute__((aligned(16))) uint32_t chords_lds[];    // [max(R.lds_words, kChordsSortWords)]
    const int tid = threadIdx.x;
    const uint64_t roi = R.roi_index ? R.roi_index[blockIdx.x] : blockIdx.x;
    if (roi >= R.n_roi)
        return;
    const uint32_t w = R.bbox_w[roi], h = R.bbox_h[roi];
    const uint32_t mn = R.min_inten[roi];
    const bool listed = chords_listed(w, h, mn, R.lds_words);
    if (listed != (R.roi_index != nullptr))
        return;                                                              // served by the other launch
    const uint64_t off = R.px_offset[roi];
    const uint64_t n64 = R.px_offset[roi + 1] - off;
    double* const o = R.out + roi * R.ld + R.col0;
    if (n64 == 0) {
        if (tid < kChordsCols) o[tid] = 0.0;
        return;
    }
    if (n64 >= 0x7FFFFFFFull || (listed && !R.ws)) {                         // (the last-writer word holds 2 * (index + 1) + 1)
        if (tid == 0) {
            atomicCAS(R.status, 0, NYXHIP_ERR_ROI_TOO_LARGE);
            for (int i = 0; i < kChordsCols; i++) o[i] = __longlong_as_double(0x7ff8000000000000LL);
        }
        return;
    }
    const uint32_t ox = R.origin_x ? R.origin_x[roi] : 0u, oy = R.origin_y ? R.origin_y[roi] : 0u;
    if (listed) {
        uint32_t* const ws = R.ws + (uint64_t)blockIdx.x * (R.ws_words + R.ws_cells);
        chords_body<true>(R, S, ws, R.ws_words, mn == 0u ? ws + R.ws_words : nullptr, R.ws_cells, chords_lds, R.x + off, R.y + off, R.inten + off,
                          (uint32_t)n64, w, h, ox, oy, o, tid);
    } else {
        chords_body<false>(R, S, chords_lds, R.lds_words, nullptr, 0, chords_lds, R.x + off, R.y + off, R.inten + off, (uint32_t)n64, w, h, ox, oy,
                           o, tid);
    }
}

__device__ bool ChordsListed::operator()(uint64_t i, uint32_t* hdr) const
{
    if (!chords_listed(bw[i], bh[i], min_inten[i], lds_words)) return false;
    const uint64_t pw = chords_plane_words(bw[i], bh[i]);
    atomicMax(&hdr[1], pw > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)pw);
    if (min_inten[i] == 0u) atomicMax(&hdr[2], chords_plane_side(bw[i], bh[i]));
    return true;
}
template int deferred_classify<ChordsListed>(uint64_t, const ChordsListed&, uint32_t*, hipStream_t);

int launch_roi_chords(const ChordArgs& a, void* stream, uint32_t grid)
{
    if (grid == 0)
        return 0;
    const uint32_t dyn = 4u * (a.lds_words > kChordsSortWords ? a.lds_words : kChordsSortWords);   // (16 .. 32 KiB)
    hipLaunchKernelGGL(roi_chords_kernel, dim3(grid), dim3(kHB), dyn, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace nyxhip
