// intensity_close.h -- the closing formulas of the first-order intensity columns: what one lane evaluates once an ROI's sums are
// known (features/intensity.cpp:67-191, moments.h:79-109 of the reference).  Every kernel that closes intensity columns calls
// these functions -- roi_features_body in the kernel, intensity_close_kernel behind it (deferred closing),
// roi_small_kernel, intensity_from_table (roi_wide, roi_large) -- so a column's arithmetic is written once and a row cannot
// depend on which kernel closed it.
//
// O is the caller's column accessor: O(I_xxx) = value.  RowColumns wraps a row pointer; intensity_close_kernel passes its packed
// LDS slots.  `blank` (all pixels zero, intensity.cpp:121-122) is an ordinary argument: the functions are force-inlined, so a
// caller that passes a constant has the branches folded away.  Guards (tid == 0, lane == 0) belong to the caller.
// Built with -ffp-contract=off (device_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "glcm_rows.h"

namespace nyxhip {

struct RowColumns {
    double* o;
    __device__ __forceinline__ double& operator()(int c) const { return o[c]; }
};

// The sums' own outputs.  tot = sum of the intensities, totsq = sum of the (32-bit wrapping) squares, mean = tot / n (the caller
// needs it anyway).  slide_range(): slide maximum - slide minimum, called only when have_slide (the arrays are optional).
template <class OUT, class SLIDE>
__device__ __forceinline__ void close_sums(const OUT& O, double dn, uint32_t vmin, uint32_t vmax, double tot, double totsq, double mean,
                                           bool have_slide, const SLIDE& slide_range, bool blank)
{
    O(I_MIN) = (double)vmin;                       // intensity.cpp:67-69
    O(I_MAX) = (double)vmax;
    O(I_RANGE) = (double)vmax - (double)vmin;
    if (have_slide)                                // intensity.cpp:72-77
        O(I_COVERED_IMAGE_INTENSITY_RANGE) = (double)(vmax - vmin) / slide_range();
    O(I_MEAN) = mean;                              // intensity.cpp:95-99
    O(I_ENERGY) = totsq;
    O(I_ROOT_MEAN_SQUARED) = sqrt(totsq / dn);
    O(I_INTEGRATED_INTENSITY) = tot;
    if (!blank)
        O(I_UNIFORMITY_PIU) = (1.0 - (double)(vmax - vmin) / (double)(uint32_t)(vmax + vmin)) * 100.0;   // :162
}

// Everything that depends only on the central sums acc = sum |d|, d^2 .. d^6 (d = value - mean): intensity.cpp:110-118, :166-191.
// Two forms with different bits -- a kernel keeps the one it has.
//
// Estimate form (roi_features, intensity_close_kernel, roi_small).  Tolerance-class outputs: the quotients and roots go through
// reciprocal / reciprocal-square-root estimates with two Newton steps (1-2 ulp) and are shared -- 1/n, 1/(n-1), 1/sqrt(variance),
// 1/sqrt(M2), 1/sqrt(n) -- instead of ten IEEE divisions and five IEEE roots on one lane (which the whole wave waits for): ~90
// instead of ~250 instructions.  A zero mean must give the reference's inf / NaN in COV, so that quotient is IEEE -- always
// (CovDiv::ieee), or only when the mean is zero (CovDiv::fast_nonzero, roi_small).
enum class CovDiv { ieee, fast_nonzero };
template <CovDiv COV, class OUT>
__device__ __forceinline__ void close_central(const OUT& O, const double (&acc)[6], uint32_t n, double dn, double mean, bool blank)
{
    const double var = acc[1];                     // intensity.cpp:110-118
    const double inv_n = frcp(dn);
    O(I_MEAN_ABSOLUTE_DEVIATION) = acc[0] * inv_n;
    const double variance = dn > 1 ? var * frcp(dn - 1) : 0.0;
    const double variance_b = dn > 1 ? var * inv_n : 0.0;
    const double rsd = variance > 0 ? frsq(variance) : 0.0;     // 1 / sd (0 stands for "sd == 0": every use below tests it)
    const double sd = variance * rsd;
    const double rs_n = frsq(dn);
    O(I_VARIANCE) = variance;
    O(I_VARIANCE_BIASED) = variance_b;
    O(I_STANDARD_DEVIATION) = sd;
    O(I_STANDARD_DEVIATION_BIASED) = variance_b > 0 ? variance_b * frsq(variance_b) : 0.0;
    O(I_COV) = (COV == CovDiv::fast_nonzero && mean != 0.0) ? fdiv(sd, mean) : sd / mean;
    O(I_STANDARD_ERROR) = sd * rs_n;
    if (!blank) {
        const double M2 = acc[1], M3 = acc[2], M4 = acc[3];     // moments.h:79-109
        if (M2 != 0.0) {
            const double r = frsq(M2), r2 = r * r;               // 1 / sqrt(M2), 1 / M2
            const double kurt = n > 4 ? (dn * M4) * (r2 * r2) : 0.0;
            O(I_SKEWNESS) = n > 3 ? ((dn * rs_n) * M3) * (r2 * r) : 0.0;   // sqrt(n) M3 / pow(M2, 1.5)
            O(I_KURTOSIS) = kurt;
            O(I_EXCESS_KURTOSIS) = n > 4 ? kurt - 3 : 0.0;
        }
        // n * pow(sd, 5), n * pow(sd, 6), intensity.cpp:186-191; a zero denominator gives 0
        const double rsd2 = rsd * rsd, t5 = inv_n * (rsd2 * rsd2 * rsd);
        O(I_HYPERSKEWNESS) = acc[4] * t5;
        O(I_HYPERFLATNESS) = acc[5] * (t5 * rsd);
    }
}

// IEEE form (intensity_from_table: roi_wide, roi_large): the reference's divisions and roots as they stand.
template <class OUT>
__device__ __forceinline__ void close_central_ieee(const OUT& O, const double (&acc)[6], uint32_t n, double dn, double mean, bool blank)
{
    O(I_MEAN_ABSOLUTE_DEVIATION) = acc[0] / dn;
    const double variance = dn > 1 ? acc[1] / (dn - 1) : 0.0, variance_b = dn > 1 ? acc[1] / dn : 0.0;
    const double sd = sqrt(variance);
    O(I_VARIANCE) = variance;
    O(I_VARIANCE_BIASED) = variance_b;
    O(I_STANDARD_DEVIATION) = sd;
    O(I_STANDARD_DEVIATION_BIASED) = sqrt(variance_b);
    O(I_COV) = sd / mean;
    O(I_STANDARD_ERROR) = sd / sqrt(dn);
    if (!blank) {
        const double M2 = acc[1], M3 = acc[2], M4 = acc[3];     // moments.h:79-109
        if (M2 != 0.0) {
            const double kurt = n > 4 ? (dn * M4) / (M2 * M2) : 0.0;
            O(I_SKEWNESS) = n > 3 ? (sqrt(dn) * M3) / (M2 * sqrt(M2)) : 0.0;
            O(I_KURTOSIS) = kurt;
            O(I_EXCESS_KURTOSIS) = n > 4 ? kurt - 3 : 0.0;
        }
        const double sd2 = sd * sd, d5 = dn * (sd2 * sd2 * sd), d6 = dn * (sd2 * sd2 * sd2);   // intensity.cpp:186-191
        O(I_HYPERSKEWNESS) = d5 == 0. ? 0. : acc[4] / d5;
        O(I_HYPERFLATNESS) = d6 == 0. ? 0. : acc[5] / d6;
    }
}

// Robust outputs of the clamped-integer sweeps of roi_features_body (offsets x = value - vmin; K values inside [p10, p90], Sx their
// exact offset sum).  First half, after sweep 1: sadk = sum |x - kmed| with kmed = m2x >> 1, m2x = 2 (median - vmin), cle =
// #(x <= kmed) when m2x is odd.
template <class OUT>
__device__ __forceinline__ void close_robust_mad(const OUT& O, double sadk, uint32_t m2x, uint32_t cle, uint32_t K, double Sx, uint32_t vmin, double dn)
{
    const double dK = (double)K;
    // sum |2x - m2x| = 2 sum |x - kmed| + (2 #(x <= kmed) - n  when m2x is odd)
    const double sadt = 2.0 * sadk + ((m2x & 1u) ? 2.0 * (double)cle - dn : 0.0);
    O(I_ROBUST_MEAN) = K ? (Sx + dK * (double)vmin) / dK : 0.0;   // exact integer sum / count, as the reference's
    O(I_MEDIAN_ABSOLUTE_DEVIATION) = fdiv(sadt * 0.5, dn);
}
// Second half, after sweep 2: adin = sum |K x - Sx| -- over the values inside [lox, hix], or (fast32) over ALL values clamped to
// that range, which the n_below / n_above values outside it are then taken out of.
template <class OUT>
__device__ __forceinline__ void close_robust_rmad(const OUT& O, double adin, bool fast32, uint32_t K, double Sx, uint32_t lox, uint32_t hix,
                                                  uint32_t n_below, uint32_t n_above)
{
    const double dK = (double)K;
    if (fast32) {                                  // (exact: every term is an integer below 2^53)
        const double klo = (double)K * (double)lox, khi = (double)K * (double)hix;
        adin -= (double)n_below * fabs(klo - Sx) + (double)n_above * fabs(khi - Sx);
    }
    O(I_ROBUST_MEAN_ABSOLUTE_DEVIATION) = K ? fdiv(fdiv(adin, dK), dK) : 0.0;
}

// intensity.cpp:137-138 (the interquartile range of histogram.h is p75 - p25)
template <class OUT>
__device__ __forceinline__ void close_quartiles(const OUT& O, double p25, double p75)
{
    O(I_QCOD) = (p75 - p25) / (p75 + p25);
    O(I_INTERQUARTILE_RANGE) = p75 - p25;
}

} // namespace nyxhip
