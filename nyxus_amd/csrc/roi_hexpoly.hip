// roi_hexpoly.hip -- the closing kernel of HexagonalityPolygonalityFeature: POLYGONALITY_AVE, HEXAGONALITY_AVE, HEXAGONALITY_STDDEV.
// A lane per ROI restates calculate() (features/hexagonality_polygonality.cpp:14-165 of the reference) operation for operation over
// six numbers other kernels left in a scratch table (roi_hexpoly.h): IEEE fp64 +, -, *, / and square roots in the reference's order,
// nothing fused -- the reference is built without FMA, and a fused a * b + c changes bits.  The 11 areas and 14 perimeters stay in
// registers: both ratio loops are fully unrolled, and the deviations come from a second pass that forms the ratios again.
#include <hip/hip_runtime.h>
#include "roi_hexpoly.h"

#pragma clang fp contract(off)

namespace nyxhip {

namespace {

constexpr double kNoValue = -1.0;                      // HexagonalityPolygonalityFeature::novalue
constexpr double kSqrt3 = 1.7320508075688772935;       // sqrt(3), correctly rounded: what the reference's sqrt(3) gives
constexpr double kPiD = 3.14159265358979323846;        // M_PI

// mean and population deviation of 1 - |1 - v[ib] / v[ic]| over ib < ic in the reference's loop order, summed one after the other
// (:84-104, :132-147).  kSkip: ratios that are not finite are left out of both passes (:91, the areas); without it a NaN or an
// infinity goes through the sums as it does in the reference (:136, the perimeters).
template <int N, bool kSkip> __device__ __forceinline__ void ratio_stats(const double (&v)[N], double& ave, double& sd)
{
    double sum = 0.0;
    uint32_t cnt = 0;
#pragma unroll
    for (int ib = 0; ib < N; ib++)
#pragma unroll
        for (int ic = ib + 1; ic < N; ic++) {
            const double r = 1.0 - fabs(1.0 - v[ib] / v[ic]);
            if (kSkip && !isfinite(r)) continue;
            cnt++;
            sum += r;
        }
    ave = sum / (double)cnt;                           // (no ratio left: 0 / 0, as in the reference)
    // The second pass divides again.  Left to itself the compiler keeps all N (N - 1) / 2 ratios of the first pass alive instead (256
    // VGPRs and 48 AGPRs, one wave per SIMD); values that have passed an empty asm statement are new to it.
    double w[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        w[k] = v[k];
        asm volatile("" : "+v"(w[k]));
    }
    double sq = 0.0;
#pragma unroll
    for (int ib = 0; ib < N; ib++)
#pragma unroll
        for (int ic = ib + 1; ic < N; ic++) {
            const double r = 1.0 - fabs(1.0 - w[ib] / w[ic]);
            if (kSkip && !isfinite(r)) continue;
            sq += (r - ave) * (r - ave);
        }
    sd = sqrt(sq / (double)cnt);
}

} // namespace

__global__ __launch_bounds__(256) void roi_hexpoly_kernel(const HexArgs A)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= A.n_roi) return;
    const double* const in = A.in + i * (uint64_t)kHexpolyInLd;
    double* const o = A.out + i * A.ld;
    const double nbd = in[kHexpolyInNumNeighbors], area_hull = in[kHexpolyInHullArea];
    // parallel_process_1_batch:202, then calculate:43-49 / :159
    const uint64_t nb = (uint64_t)nbd;
    if (A.n_contour[i] == 0 || area_hull == 0.0 || nbd == 0.0 || nb < 3) {
        o[0] = kNoValue; o[1] = kNoValue; o[2] = kNoValue;
        return;
    }
    const double neighbors = (double)nb;
    const double area = (double)(A.px_offset[i + 1] - A.px_offset[i]);
    const double perimeter = in[kHexpolyInPerimeter];
    const double min_feret = in[kHexpolyInFeretMin], max_feret = in[kHexpolyInFeretMax];
    const double perim_hull = 6.0 * sqrt(area_hull / (1.5 * kSqrt3));
    const double perimeter_neighbors = perimeter / neighbors;
    const double t = nb <= (uint64_t)kHexpolyTanCap ? A.tan_tab[nb] : tan(kPiD / neighbors);
    // ---- polygonality (:51-55)
    const double poly_size_ratio = 1.0 - fabs(1.0 - perimeter_neighbors / sqrt((4.0 * area) / (neighbors / t)));
    const double poly_area_ratio = 1.0 - fabs(1.0 - area / (0.25 * neighbors * perimeter_neighbors * perimeter_neighbors / t));
    const double poly_ave = 10.0 * (poly_size_ratio + poly_area_ratio) / 2.0;
    // ---- hexagonality (:58-152)
    const double apoth1 = kSqrt3 * perimeter / 12.0, apoth2 = kSqrt3 * max_feret / 4.0, apoth3 = min_feret / 2.0;
    const double side1 = perimeter / 6.0, side2 = max_feret / 2.0, side3 = min_feret / kSqrt3, side4 = perim_hull / 6.0;
    const double hex = 0.5 * (3.0 * kSqrt3);
    double area_ave, area_sd, perim_ave, perim_sd;
    {
        const double list_area[11] = {hex * side1 * side1, hex * side2 * side2, hex * side3 * side3, 3.0 * side1 * apoth2, 3.0 * side1 * apoth3,
                                      3.0 * side2 * apoth3, 3.0 * side4 * apoth1, 3.0 * side4 * apoth2, 3.0 * side4 * apoth3, area_hull, area};
        ratio_stats<11, true>(list_area, area_ave, area_sd);
    }
    {
        const double apoth4 = kSqrt3 * perim_hull / 12.0, apoth5 = sqrt(4.0 * area_hull / (4.5 * kSqrt3));
        const double list_perim[14] = {sqrt(24.0 * area / kSqrt3), sqrt(24.0 * area_hull / kSqrt3), perimeter, perim_hull, 3.0 * max_feret,
                                       6.0 * min_feret / kSqrt3, 2.0 * area / apoth1, 2.0 * area / apoth2, 2.0 * area / apoth3, 2.0 * area / apoth4,
                                       2.0 * area / apoth5, 2.0 * area_hull / apoth1, 2.0 * area_hull / apoth2, 2.0 * area_hull / apoth3};
        ratio_stats<14, false>(list_perim, perim_ave, perim_sd);
    }
    o[0] = poly_ave;
    o[1] = 10.0 * (area_ave + perim_ave) / 2.0;
    o[2] = sqrt((area_sd * area_sd + perim_sd * perim_sd) / 2.0);
}

int launch_roi_hexpoly(const HexArgs& a, void* stream)
{
    if (a.n_roi == 0)
        return 0;
    hipLaunchKernelGGL(roi_hexpoly_kernel, dim3((unsigned)((a.n_roi + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace nyxhip
