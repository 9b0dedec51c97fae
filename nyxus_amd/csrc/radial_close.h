// radial_close.h -- what every radial-distribution kernel shares beyond the hill descent (contour_descent.h): the wedge of a direction,
// the host's table for the eight boundary directions, and the tail that turns the integer bins of one ring into FRAC_AT_D, MEAN_FRAC
// and RADIAL_CV (radial_distribution.cpp:90-96, :212-247).  Used by roi_radial.hip (a workgroup per ROI) and roi_wsgroup.hip (whole slides).
#pragma once
#include <stdint.h>
#include <cmath>
#include <algorithm>
#include "roi_radial.h"

namespace nyxhip {

// The wedge of the eight directions that lie ON an octant boundary (k * 45 degrees, four bits each): the reference expression
// (radial_distribution.cpp:92-96) on the host's libm, as the reference evaluates it; every other direction is an exact integer test.
inline uint32_t radial_wedge_tab()
{
    static const int kDirX[8] = {1, 1, 0, -1, -1, -1, 0, 1}, kDirY[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    const double two_pi = 2.0 * 3.14159265358979323846;
    uint32_t tab = 0;
    for (int k = 0; k < 8; k++) {
        double ang = std::atan2((double)kDirY[k], (double)kDirX[k]);
        if (ang < 0) ang = two_pi + ang;
        const double angW = two_pi / double(kRadialBins);
        const int w_bin = std::min(std::max(int(ang / angW), 0), kRadialBins - 1);
        tab |= (uint32_t)w_bin << (4 * k);
    }
    return tab;
}

#if defined(__HIPCC__)
// int(ang / (2 pi / 8)), ang = atan2(dy, dx) [+ 2 pi if negative] (radial_distribution.cpp:90-96) for integer dx, dy.
// Octant k covers [k, k + 1) * 45 degrees.  A direction off the eight boundary directions is at least 1e-10 rad away from one
// (|dx|, |dy| < 2^16), eleven orders above the rounding of atan2 and of the division: its bin is the octant it lies in.
__device__ __forceinline__ int wedge_of(int dx, int dy, uint32_t tab)
{
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    if ((ax | ay) == 0) return 0;                                        // atan2(0, 0) = 0
    if (ay == 0) return (int)((tab >> (dx > 0 ? 0 : 16)) & 15u);         // 0, 180 degrees
    if (ax == 0) return (int)((tab >> (dy > 0 ? 8 : 24)) & 15u);         // 90, 270
    if (ax == ay) {
        const int k = dy > 0 ? (dx > 0 ? 1 : 3) : (dx < 0 ? 5 : 7);      // 45, 135, 225, 315
        return (int)((tab >> (4 * k)) & 15u);
    }
    if (dy > 0) return dx > 0 ? (ax > ay ? 0 : 1) : (ax < ay ? 2 : 3);
    return dx < 0 ? (ax > ay ? 4 : 5) : (ax < ay ? 6 : 7);
}

// The ring of a pixel at (dx, dy) from the centre whose largest contour distance is dstOC (:74-88): sqrt, divide, multiply, truncate
__device__ __forceinline__ int ring_of(int dx, int dy, double dstOC)
{
    const double ddx = (double)dx, ddy = (double)dy;
    const double dstOA = sqrt(ddx * ddx + ddy * ddy);                     // exact integer below 2^53 under the root
    const double rat = dstOA / dstOC;
    int ring = (int)(rat * (double)(kRadialBins - 1));                    // 0 <= rat < 2^17: the conversion is defined
    if (ring >= kRadialBins) ring = kRadialBins - 1;
    return ring;
}

// get_FracAtD, get_MeanFrac, get_RadialCV (:212-247) of one ring: cnt pixels, wsum[k] the intensity sum of its wedge k, n the ROI's pixels
__device__ __forceinline__ void radial_tail(double cnt, const unsigned long long (&wsum)[kRadialBins], double n, double& frac, double& mean_frac, double& cv)
{
    const double epsilon = 0.000000001;                                   // radial_distribution.h:71
    unsigned long long isum = 0;
#pragma unroll
    for (int k = 0; k < kRadialBins; k++) isum += wsum[k];                // radial_intensity_bins[ring]: the same pixels, summed exactly
    frac = cnt / (n + epsilon);
    mean_frac = (double)isum / (cnt + epsilon);
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < kRadialBins; k++) sum += (double)wsum[k];
    const double mean = sum / (double)kRadialBins;
    sum = 0;
#pragma unroll
    for (int k = 0; k < kRadialBins; k++) sum += ((double)wsum[k] - mean) * ((double)wsum[k] - mean);
    const double var = sum / (double)kRadialBins;
    cv = sqrt(var) / (mean + epsilon);
}
#endif

} // namespace nyxhip
