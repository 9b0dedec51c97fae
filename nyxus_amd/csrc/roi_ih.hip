// roi_ih.hip -- the reference's IBSI intensity-histogram class on the device:
//   IntensityHistogramFeatures   IH_MEAN_VAL .. IH_BIN_SIZE, 46 columns    features/intensity_histogram.cpp:29-325 (of the reference)
//
//   roi_ih_kernel<1>         A wave per ROI, kIhWaves ROIs per workgroup (the waves never meet: no workgroup barrier), for ROIs of at
//                            most IhArgs::wave_px pixels.
//   roi_ih_kernel<kIhWaves>  A workgroup per ROI above that; wave 0 closes.
//   Both stream the ROI's intensities once from HBM.  LDS holds nothing but the N uint32 counters of the ROI (dynamic LDS, sized from N;
//   32 bits: one bin of a large flat ROI exceeds 65535), so there is no path "beyond LDS" and no size class.
//   Binning    idx = (int) floor((v - mn) / binWidth), clamped to [0, N - 1]: the reference's expression in fp64, as written (fp64
//              division is correctly rounded, -ffp-contract=off).  Plain LDS atomic adds.
//   Scan       one pass over the bins, 64 at a time: integer prefix sums of the counts (the reference's running fp64 sums of counts are
//              integers below 2^53, so a prefix sum converted once has their bits); the bins at which the reference's loops stop (median,
//              the four quantiles with their two scan directions) come from the reference's own comparisons, evaluated per bin and
//              picked with a ballot -- C / total is monotone in C, so "first bin at which the loop condition fails" is a first (or
//              last) set bit; mode = first largest bin; gradient extremes in integers (twice the gradient).
//   Sums       the per-bin terms of the reference's two loops are computed a lane per bin and ADDED ONE AFTER THE OTHER in bin order
//              (as roi_circle.hip does for the perimeter): the sums carry the reference's bits.  A term the reference skips is added
//              as +0.0, which leaves a sum that started at +0.0 unchanged.  Every term of an EMPTY bin is +-0.0 (its probability is 0), and
//              a sum that started at +0.0 is never -0.0, so the adds of empty bins are left out: the bins with pixels are walked through
//              a ballot.  A 49-px ROI fills at most 49 of 64 bins, a flat ROI two or three.
//   Entropy    log() is the device library's, the reference's is glibc's: the two entropy columns agree to rounding, every other
//              column bit for bit.
//   Integer images only: float_domain_map (intensity_histogram.cpp:331-372) is scale 1, offset 0 unless the slide is a float image or
//   HU mode is on, and neither exists behind this ABI.
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_ih.h"

namespace nyxhip {

namespace {

__device__ __forceinline__ double lane_value(double v, int t)                  // v of lane t (t wave-uniform)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), t), hi = __builtin_amdgcn_readlane(__double2hiint(v), t);
    return __hiloint2double(hi, lo);
}

// (int) of a double as x86-64 converts it (cvttsd2si: INT_MIN for NaN and whatever lies outside int), then the reference's clamp
__device__ __forceinline__ int bin_of(double q, int N)
{
    int idx = (q >= -2147483648.0 && q < 2147483648.0) ? (int)q : (-2147483647 - 1);
    if (idx < 0) idx = 0;
    if (idx >= N) idx = N - 1;
    return idx;
}

struct Stop {                  // a bin at which one of the reference's scans stops
    int j;                     // the bin (-1: not met yet)
    uint32_t f;                // its count
    uint64_t c;                // ascending scans: the counts in front of it; descending scans: the counts behind it
};

// The closing computation of one ROI by one wave.  F: the N counters.
__device__ __forceinline__ void ih_close(const uint32_t* F, int N, uint32_t n, double mn, double mx, double bw, double* row, int lane)
{
    const double tot = (double)n;
    const uint64_t half = n / 2;                                               // count / 2, integer division (medianFromBins)
    auto bin_center = [&](int i) { return mn + ((double)i + 0.5) * bw; };
    auto bin_min = [&](int i) { return mn + (double)i * bw; };
    auto bin_max = [&](int i) { return mn + (double)(i + 1) * bw; };
    auto index_of = [&](double v) { return bin_of(floor((v - mn) / bw), N); };

    // ---- scan: stop bins, mode, gradient extremes ------------------------------------------------------------------------------
    int jmed = -1;
    Stop q10{-1, 0, 0}, q25{-1, 0, 0}, q75{-1, 0, 0}, q90{-1, 0, 0};
    uint32_t mode_f = 0; int mode_i = 0;
    long long gmax2 = 0, gmin2 = 0x7FFFFFFFFFFFFFFFLL; int gmax_i = -1, gmin_i = -1;   // twice the gradient; gmax2 = 0: "> DBL_MIN" is "> 0"
    uint64_t carry = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool valid = i < N;
        const uint32_t f = valid ? F[i] : 0u;
        uint64_t inc = f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        inc += carry;
        const uint64_t cex = inc - f;
        carry = __shfl(inc, 63, 64);
        if (jmed < 0) {                                                        // while (total <= half): stops behind the first bin with total > half
            const unsigned long long m = __ballot(valid && inc > half);
            if (m) jmed = base + (__ffsll((long long)m) - 1);
        }
        auto ascending = [&](Stop& s, double p) {                              // do .. while (n < N && p_n < p)
            if (s.j >= 0) return;
            const unsigned long long m = __ballot(valid && !((double)inc / tot < p));
            if (m) { const int l = __ffsll((long long)m) - 1; s.j = base + l; s.f = __shfl(f, l, 64); s.c = __shfl(cex, l, 64); }
        };
        auto descending = [&](Stop& s, double p) {                             // do .. while (m < N && p_n > p), from the last bin down
            const unsigned long long m = __ballot(valid && !(1.0 - (double)((uint64_t)n - cex) / tot > p));
            if (m) { const int l = 63 - __clzll((long long)m); s.j = base + l; s.f = __shfl(f, l, 64); s.c = (uint64_t)n - __shfl(inc, l, 64); }
        };
        ascending(q10, 0.10); ascending(q25, 0.25);
        descending(q75, 0.75); descending(q90, 0.90);
        // mode: if (modeFrequence < f), in bin order
        uint32_t fm = f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) fm = max(fm, (uint32_t)__shfl_xor(fm, o, 64));
        if (fm > mode_f) { mode_f = fm; mode_i = base + (__ffsll((long long)__ballot(valid && f == fm)) - 1); }
        // gradient: freq[1] - freq[0] | freq[N-1] - freq[N-2] | (freq[i+1] - freq[i-1]) / 2
        long long g2 = 0;
        if (valid) {
            if (i == 0) g2 = 2 * ((long long)F[1] - (long long)F[0]);
            else if (i == N - 1) g2 = 2 * ((long long)F[i] - (long long)F[i - 1]);
            else g2 = (long long)F[i + 1] - (long long)F[i - 1];
        }
        long long gx = valid ? g2 : (-0x7FFFFFFFFFFFFFFFLL - 1), gn = valid ? g2 : 0x7FFFFFFFFFFFFFFFLL;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { gx = max(gx, (long long)__shfl_xor(gx, o, 64)); gn = min(gn, (long long)__shfl_xor(gn, o, 64)); }
        if (gx > gmax2) { gmax2 = gx; gmax_i = base + (__ffsll((long long)__ballot(valid && g2 == gx)) - 1); }
        if (gn < gmin2) { gmin2 = gn; gmin_i = base + (__ffsll((long long)__ballot(valid && g2 == gn)) - 1); }
    }
    if (jmed < 0) jmed = N - 1;

    // ---- values and their bins (intensity_histogram.cpp:68-128) -------------------------------------------------------------------
    auto q_low = [&](const Stop& s, double p) {
        const double p_prev = (double)s.c / tot, prop = (double)s.f / tot, lo = bin_min(s.j), hi = bin_max(s.j), interval = hi - lo;
        return lo + ((p - p_prev) / prop) * interval;
    };
    auto q_high = [&](const Stop& s, double p) {
        const double p_prev = 1.0 - (double)s.c / tot, prop = (double)s.f / tot, lo = bin_min(s.j), hi = bin_max(s.j), interval = hi - lo;
        return hi - ((p_prev - p) / prop) * interval;
    };
    const double med_v = bin_center(jmed);
    const int med_i = index_of(med_v);
    const int min_i = index_of(mn), max_i = index_of(mx);
    const double p10_v = q_low(q10, 0.10), p25_v = q_low(q25, 0.25), p75_v = q_high(q75, 0.75), p90_v = q_high(q90, 0.90);
    const int p10_i = index_of(p10_v), p25_i = index_of(p25_v), p75_i = index_of(p75_v), p90_i = index_of(p90_v);

    // ---- first loop: mean, robust mean over [p10_i, p90_i] --------------------------------------------------------------------------
    double mean_v = 0.0, mean_i = 0.0, rsum_v = 0.0;
    uint64_t rcount = 0, rsum_i = 0;                                           // sums of integers below 2^53: exact in the reference's fp64 as well
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool valid = i < N;
        const uint32_t f = valid ? F[i] : 0u;
        const double prob = (double)f / tot, vv = bin_center(i);
        const bool in = valid && i >= p10_i && i <= p90_i;
        const double t0 = valid ? prob * vv : 0.0, t1 = valid ? prob * (double)i : 0.0, t2 = in ? (double)f * vv : 0.0;
        uint64_t rc = in ? f : 0u, ri = in ? (uint64_t)f * (uint64_t)i : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { rc += __shfl_xor(rc, o, 64); ri += __shfl_xor(ri, o, 64); }
        rcount += rc; rsum_i += ri;
        for (unsigned long long m = __ballot(f != 0u); m; m &= m - 1) {        // the reference's order: one dependent add per bin (empty bins: +-0)
            const int t = __ffsll((long long)m) - 1;
            mean_v += lane_value(t0, t);
            mean_i += lane_value(t1, t);
            rsum_v += lane_value(t2, t);
        }
    }
    const double rcount_d = (double)rcount;
    const double rmean_v = rsum_v / rcount_d, rmean_i = (double)rsum_i / rcount_d;

    // ---- second loop ------------------------------------------------------------------------------------------------------------
    constexpr int kSums = 14;
    constexpr double kLog2 = 0.69314718055994530942;                           // std::log(2.0)
    double S[kSums];
#pragma unroll
    for (int c = 0; c < kSums; c++) S[c] = 0.0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool valid = i < N;
        const uint32_t f = valid ? F[i] : 0u;
        const double fd = (double)f, prob = fd / tot, vv = bin_center(i), id = (double)i;
        const double dv = vv - mean_v, di = id - mean_i;
        const bool in = valid && i >= p10_i && i <= p90_i;
        double T[kSums];
        T[0] = prob * dv * dv;                                                 // variance
        T[1] = prob * di * di;
        T[2] = prob * dv * dv * dv;                                            // skewness
        T[3] = prob * di * di * di;
        T[4] = prob * dv * dv * dv * dv;                                       // kurtosis
        T[5] = prob * di * di * di * di;
        T[6] = prob * fabs(dv);                                                // mean absolute deviation
        T[7] = prob * fabs(di);
        T[8] = in ? fd * fabs(vv - rmean_v) : 0.0;                             // robust mean absolute deviation
        T[9] = in ? fd * fabs(id - rmean_i) : 0.0;
        T[10] = prob * fabs(vv - med_v);                                       // median absolute deviation
        T[11] = prob * fabs(id - (double)med_i);
        T[12] = prob > 0.0000001 ? -(prob * log(prob) / kLog2) : 0.0;          // entropy: value -= term
        T[13] = prob * prob;                                                   // uniformity
        if (!valid) {
#pragma unroll
            for (int c = 0; c < kSums; c++) T[c] = 0.0;
        }
        for (unsigned long long m = __ballot(f != 0u); m; m &= m - 1) {
            const int t = __ffsll((long long)m) - 1;
#pragma unroll
            for (int c = 0; c < kSums; c++) S[c] += lane_value(T[c], t);
        }
    }
    if (lane != 0)
        return;
    const double var_v = S[0], var_i = S[1];
    const double skew_v = S[2] / (var_v * sqrt(var_v)), skew_i = S[3] / (var_i * sqrt(var_i));
    const double kurt_v = S[4] / (var_v * var_v) - 3.0, kurt_i = S[5] / (var_i * var_i) - 3.0;
    const double cov_v = sqrt(var_v) / mean_v, cov_i = sqrt(var_i) / (mean_i + 1.0);
    const double qcod_v = (p75_v - p25_v) / (p75_v + p25_v);
    const double qcod_i = ((double)p75_i - (double)p25_i) / ((double)p75_i + 1.0 + (double)p25_i + 1.0);
    const double rmad_v = S[8] / rcount_d, rmad_i = S[9] / rcount_d;
    // value family (20)
    row[0] = mean_v; row[1] = var_v; row[2] = skew_v; row[3] = kurt_v; row[4] = med_v; row[5] = mn; row[6] = p10_v; row[7] = p90_v;
    row[8] = mx; row[9] = bin_center(mode_i); row[10] = p75_v - p25_v; row[11] = mx - mn; row[12] = S[6]; row[13] = rmad_v;
    row[14] = S[10]; row[15] = cov_v; row[16] = qcod_v; row[17] = S[12]; row[18] = S[13]; row[19] = rmean_v;
    // index family (19): bin indices are 1-based; variance, skewness and kurtosis are not shifted; entropy and uniformity are copies
    row[20] = mean_i + 1.0; row[21] = var_i; row[22] = skew_i; row[23] = kurt_i; row[24] = (double)med_i + 1.0;
    row[25] = (double)min_i + 1.0; row[26] = (double)p10_i + 1.0; row[27] = (double)p90_i + 1.0; row[28] = (double)max_i + 1.0;
    row[29] = (double)mode_i + 1.0; row[30] = (double)p75_i - (double)p25_i; row[31] = (double)max_i - (double)min_i; row[32] = S[7];
    row[33] = rmad_i; row[34] = S[11]; row[35] = cov_i; row[36] = qcod_i; row[37] = S[12]; row[38] = S[13];
    // gradient + bookkeeping (7).  The maximum is seeded with numeric_limits<double>::min(): without a positive gradient it stays, index 0
    row[39] = gmax_i < 0 ? 2.2250738585072014e-308 : (double)gmax2 / 2.0;
    row[40] = gmax_i < 0 ? 0.0 : (double)(gmax_i + 1);
    row[41] = (double)gmin2 / 2.0;
    row[42] = (double)(gmin_i + 1);
    row[43] = rmean_i + 1.0; row[44] = (double)N; row[45] = bw;
}

} // namespace

template <int TEAM>
__global__ __launch_bounds__(64 * kIhWaves) void roi_ih_kernel(const IhArgs A)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t ih_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t roi = TEAM == 1 ? (uint64_t)blockIdx.x * kIhWaves + (uint64_t)wave : (uint64_t)blockIdx.x;
    if (roi >= A.n_roi)
        return;
    const uint64_t off = A.px_offset[roi];
    const uint32_t n = (uint32_t)(A.px_offset[roi + 1] - off);
    if ((n <= A.wave_px) != (TEAM == 1))
        return;                                                               // the other form's ROI (uniform over the team)
    double* const row = A.out + roi * A.ld;
    const int N = A.n_bins;
    const uint32_t vmn = A.vmin[roi], vmx = A.vmax[roi];
    if (!A.ibsi || vmx <= vmn || N < 2 || n == 0) {                           // intensity_histogram.cpp:304-320
        if (wave == 0 || TEAM == 1)
            for (int c = lane; c < kIhCols; c += 64) row[c] = A.soft_nan;
        return;
    }
    uint32_t* const F = ih_lds + (TEAM == 1 ? (size_t)wave * (size_t)N : (size_t)0);
    const uint32_t tid = TEAM == 1 ? (uint32_t)lane : threadIdx.x;
    constexpr uint32_t kThreads = 64u * TEAM;
    for (uint32_t i = tid; i < (uint32_t)N; i += kThreads) F[i] = 0u;
    if (TEAM == 1) wav_sync<false>(); else __syncthreads();
    const double mn = (double)vmn, mx = (double)vmx, bw = (mx - mn) / (double)N;
    const uint32_t* const V = A.inten + off;
    for (uint32_t i = tid; i < n; i += kThreads)
        atomicAdd(&F[bin_of(floor(((double)V[i] - mn) / bw), N)], 1u);
    if (TEAM == 1) wav_sync<false>(); else __syncthreads();
    if (TEAM != 1 && wave != 0)
        return;
    ih_close(F, N, n, mn, mx, bw, row, lane);
}

int launch_roi_ih(const IhArgs& a, void* stream, bool wave_form, bool block_form)
{
    if (a.n_roi == 0)
        return 0;
    if (a.ibsi && a.n_bins > kIhMaxBins)
        return (int)hipErrorInvalidValue;                                     // (the entries refuse it with a message of their own)
    const uint32_t bins = a.ibsi && a.n_bins > 0 ? (uint32_t)a.n_bins : 0u;   // (a gated call touches no LDS)
    if (wave_form) {
        hipLaunchKernelGGL(roi_ih_kernel<1>, dim3((uint32_t)((a.n_roi + kIhWaves - 1) / kIhWaves)), dim3(64 * kIhWaves), (size_t)kIhWaves * 4u * bins,
                           (hipStream_t)stream, a);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    if (block_form) {
        hipLaunchKernelGGL(roi_ih_kernel<kIhWaves>, dim3((uint32_t)a.n_roi), dim3(64 * kIhWaves), (size_t)4u * bins, (hipStream_t)stream, a);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}

} // namespace nyxhip
