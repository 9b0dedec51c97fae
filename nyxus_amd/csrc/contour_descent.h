// contour_descent.h -- the reference's hill descent of a pixel over the ORDERED contour (Pixel2::min_sqdist / max_sqdist v2,
// features/pixel.cpp:40-70, :116-143), shared by the moments kernel (roi_moments.hip) and the radial distribution kernel
// (roi_radial.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace nyxhip {

// (int)(m / log(m)) for the window widths m the hill descent meets; m <= 10 -> 1 (pixel.cpp:47,66)
__device__ __forceinline__ int descent_step(size_t m, const uint16_t* tab, int tab_n)
{
    if (m <= 10) return 1;
    if ((int)m < tab_n) return (int)tab[m];
    return (int)((double)m / log((double)m));
}

// Pixel2::min_sqdist v2 (pixel.cpp:40-70) and, with MAX, Pixel2::max_sqdist v2 (pixel.cpp:116-143: the same descent with the
// comparison flipped): hill descent over the ordered contour.  step0 = (int)(n / log(n)).
// SMALL: every coordinate is below 2^15, so the squared distances are exact in 32-bit integers (24-bit multiplies) and the
// whole search runs on integer compares; otherwise the distances are formed in double like the reference's.  The index
// arithmetic is 32-bit either way (a contour has fewer points than the ROI has pixels).
// (n == 1: the reference's first step is (int)(1 / log(1)) -- a conversion of infinity; the single point's distance is returned.)
template <bool SMALL, bool MAX>
__device__ __forceinline__ double sqdist_descent(int px, int py, const uint32_t* K, int n, int step0, const uint16_t* tab, int tab_n)
{
    if (n == 0) return 0.0;
    using dist_t = typename std::conditional<SMALL, uint32_t, double>::type;
    const uint32_t ppack = ((uint32_t)px & 0xFFFFu) | ((uint32_t)py << 16);
    auto sqd = [&](uint32_t i) -> dist_t {
        const uint32_t k = K[i];
        if (SMALL) {
            // a contour point is x | y << 16 and both coordinates are below 2^15: the difference is one packed 16-bit subtraction,
            // dx^2 + dy^2 one two-element dot product (v_pk_sub_i16 + v_dot2_i32_i16 instead of unpack / subtract / square / add)
            typedef short s16x2 __attribute__((ext_vector_type(2)));
            const s16x2 d = __builtin_bit_cast(s16x2, k) - __builtin_bit_cast(s16x2, ppack);
            return (dist_t)(uint32_t)__builtin_amdgcn_sdot2(d, d, 0, false);
        } else {
            const double dx = (double)(int)(k & 0xFFFFu) - (double)px, dy = (double)(int)(k >> 16) - (double)py;
            return (dist_t)(dx * dx + dy * dy);
        }
    };
    dist_t extrem_d = sqd(0);
    if (n == 1) return (double)extrem_d;
    uint32_t a = 0, b = (uint32_t)n, extrem_i = 0;
    uint32_t step = (uint32_t)step0;
    do {
        for (uint32_t i = a + step; i < b; i += step) {
            const dist_t d = sqd(i);
            if (MAX ? extrem_d < d : extrem_d > d) { extrem_d = d; extrem_i = i; }
        }
        const uint32_t stepL = extrem_i >= step ? step : extrem_i,
                       stepR = extrem_i + step < (uint32_t)n ? step : (uint32_t)n - extrem_i;
        a = extrem_i - stepL;
        b = extrem_i + stepR;
        step = (uint32_t)descent_step((size_t)(b - a), tab, tab_n);
    } while (b - a > 2);
    return (double)extrem_d;
}

template <bool SMALL>
__device__ __forceinline__ double min_sqdist_v2(int px, int py, const uint32_t* K, int n, int step0, const uint16_t* tab, int tab_n)
{
    return sqdist_descent<SMALL, false>(px, py, K, n, step0, tab, tab_n);
}

template <bool SMALL>
__device__ __forceinline__ double max_sqdist_v2(int px, int py, const uint32_t* K, int n, int step0, const uint16_t* tab, int tab_n)
{
    return sqdist_descent<SMALL, true>(px, py, K, n, step0, tab, tab_n);
}

} // namespace nyxhip
