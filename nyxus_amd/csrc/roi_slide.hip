// roi_slide.hip -- whole-slide mode: every slide of a stack is one ROI with label 1 that covers the whole image (gfx950).
//
// The reference's virtual ROI (the reference's src/nyx/workflow_2d_whole.cpp:36-213, slideprops.cpp:101-254): area = width * height,
// box = the image with origin (0, 0), aux_min / aux_max = the extrema over ALL pixels (zero-valued ones included), which are the
// slide's extrema as well, pixel order row-major.
//
//   slide_extrema_kernel  one workgroup per slab of a slide's pixels: 16-byte loads in the image's own element type, a wave
//                         reduction, one atomicMin and one atomicMax per workgroup into the slide's header
//   slide_header_kernel   one thread per slide: the per-ROI arrays of a nyxhip_batch (CSR offsets, box, extrema, slide extrema, label)
//   slide_cloud_kernel    the row-major cloud (u16 x, u16 y, u32 intensity) of every slide: what the size-class kernels of every
//                         family read
//
// Built with -ffp-contract=off (device_math.h).
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_kernel.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

template <typename T>
__device__ __forceinline__ void word_minmax(uint32_t wd, uint32_t& lo, uint32_t& hi)
{
    if constexpr (sizeof(T) == 4) {
        lo = wd < lo ? wd : lo; hi = wd > hi ? wd : hi;
    } else if constexpr (sizeof(T) == 2) {
        const uint32_t a = wd & 0xFFFFu, b = wd >> 16;
        lo = a < lo ? a : lo; hi = a > hi ? a : hi;
        lo = b < lo ? b : lo; hi = b > hi ? b : hi;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t a = (wd >> (8 * k)) & 0xFFu;
            lo = a < lo ? a : lo; hi = a > hi ? a : hi;
        }
    }
}

// grid (slabs of a slide, slides).  vmin / vmax: [n_slides], preset to 0xFFFFFFFF / 0.
template <typename T>
__global__ __launch_bounds__(256) void slide_extrema_kernel(const T* __restrict__ img, uint64_t px, uint32_t slab, uint32_t* __restrict__ vmin,
                                                            uint32_t* __restrict__ vmax)
{
    constexpr uint32_t EPV = 16 / sizeof(T);                                  // elements of a 16-byte load
    __shared__ uint32_t s_lo[4], s_hi[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t t = blockIdx.y;
    const T* const p = img + (uint64_t)t * px;
    const uint64_t s0 = (uint64_t)blockIdx.x * slab, s1 = s0 + slab < px ? s0 + slab : px;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    if (s0 < s1) {
        // [s0, e0) element by element up to the first 16-byte boundary, [e0, e1) as vectors, [e1, s1) element by element.  A slab of a
        // slide starts anywhere: an odd pixel count per slide, or the chunk's offset inside the caller's array.
        const uintptr_t a = (uintptr_t)(p + s0);
        uint64_t head = (a % sizeof(T)) ? s1 - s0 : (uint64_t)(((16u - (uint32_t)(a & 15u)) & 15u) / sizeof(T));
        if (head > s1 - s0) head = s1 - s0;
        const uint64_t e0 = s0 + head, nv = (s1 - e0) / EPV, e1 = e0 + nv * EPV;
        const uint4* const v = (const uint4*)(p + e0);
        for (uint64_t i = tid; i < nv; i += 256) {
            const uint4 q = v[i];
            word_minmax<T>(q.x, lo, hi); word_minmax<T>(q.y, lo, hi); word_minmax<T>(q.z, lo, hi); word_minmax<T>(q.w, lo, hi);
        }
        for (uint64_t i = s0 + tid; i < e0; i += 256) { const uint32_t x = p[i]; lo = x < lo ? x : lo; hi = x > hi ? x : hi; }
        for (uint64_t i = e1 + tid; i < s1; i += 256) { const uint32_t x = p[i]; lo = x < lo ? x : lo; hi = x > hi ? x : hi; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t ol = (uint32_t)__shfl_xor((int)lo, d, 64), oh = (uint32_t)__shfl_xor((int)hi, d, 64);
        lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
    }
    if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; k++) { lo = s_lo[k] < lo ? s_lo[k] : lo; hi = s_hi[k] > hi ? s_hi[k] : hi; }
        if (lo <= hi) { atomicMin(&vmin[t], lo); atomicMax(&vmax[t], hi); }
    }
}

__global__ __launch_bounds__(256) void slide_header_kernel(SlideRows R, uint32_t n, uint64_t px, uint32_t w, uint32_t h)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t > n) return;
    R.px_offset[t] = (uint64_t)t * px;
    if (t == n) return;
    R.label[t] = 1u;                                                          // the virtual ROI's label (workflow_2d_whole.cpp)
    R.bbox_w[t] = w; R.bbox_h[t] = h;
    R.slide_min[t] = (double)R.vmin[t];                                       // the slide's extrema are the ROI's: the ROI is the slide
    R.slide_max[t] = (double)R.vmax[t];
}

// grid (groups of 1024 pixels of a slide, slides first .. first + grid.y of the chunk): a thread takes four consecutive pixels of the
// slide's row-major order.  img, cx, cy, cv: the chunk's arrays (slide t owns [t * px, (t + 1) * px) of each).
template <typename T>
__global__ __launch_bounds__(256) void slide_cloud_kernel(const T* __restrict__ img, uint64_t px, uint32_t w, uint32_t first, uint16_t* __restrict__ cx,
                                                          uint16_t* __restrict__ cy, uint32_t* __restrict__ cv)
{
    const uint64_t j0 = 4ull * ((uint64_t)blockIdx.x * 256u + threadIdx.x);
    if (j0 >= px) return;
    const uint64_t base = ((uint64_t)first + blockIdx.y) * px;                // the slide's first pixel in the chunk's image and cloud
    const T* const p = img + base;
    uint32_t x = (uint32_t)(j0 % w), y = (uint32_t)(j0 / w);
    const uint32_t m = px - j0 < 4 ? (uint32_t)(px - j0) : 4u;
    uint32_t xs[4], ys[4], vs[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        xs[k] = x; ys[k] = y; vs[k] = k < m ? (uint32_t)p[j0 + k] : 0u;
        if (++x == w) { x = 0; y++; }
    }
    const uint64_t g = base + j0;
    if (m == 4 && (g & 3ull) == 0) {                                          // (the arrays are 256-byte aligned: a multiple of four is a vector)
        *(uint2*)(cx + g) = make_uint2(xs[0] | (xs[1] << 16), xs[2] | (xs[3] << 16));
        *(uint2*)(cy + g) = make_uint2(ys[0] | (ys[1] << 16), ys[2] | (ys[3] << 16));
        *(uint4*)(cv + g) = make_uint4(vs[0], vs[1], vs[2], vs[3]);
    } else
        for (uint32_t k = 0; k < m; k++) { cx[g + k] = (uint16_t)xs[k]; cy[g + k] = (uint16_t)ys[k]; cv[g + k] = vs[k]; }
}

template <typename T>
int extrema_and_header(const void* inten, uint32_t w, uint32_t h, uint32_t n, SlideRows R, hipStream_t st)
{
    const uint64_t px = (uint64_t)w * h;
    const uint32_t slab = 256u * 4u * (16u / (uint32_t)sizeof(T));          // four 16-byte loads per thread
    hipLaunchKernelGGL(slide_extrema_kernel<T>, dim3((unsigned)((px + slab - 1) / slab), n), dim3(256), 0, st, (const T*)inten, px, slab, R.vmin, R.vmax);
    hipLaunchKernelGGL(slide_header_kernel, dim3(n / 256 + 1), dim3(256), 0, st, R, n, px, w, h);
    return (int)hipGetLastError();
}

template <typename T>
int clouds(const void* inten, uint32_t w, uint32_t h, uint32_t first, uint32_t n, uint16_t* cx, uint16_t* cy, uint32_t* cv, hipStream_t st)
{
    const uint64_t px = (uint64_t)w * h;
    hipLaunchKernelGGL(slide_cloud_kernel<T>, dim3((unsigned)((px + 1023) / 1024), n), dim3(256), 0, st, (const T*)inten, px, w, first, cx, cy, cv);
    return (int)hipGetLastError();
}

} // namespace

int launch_slide_headers(const void* inten, int dt_inten, uint32_t w, uint32_t h, uint32_t n_slides, SlideRows R, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(R.vmin, 0xFF, 4ull * n_slides, st); e != hipSuccess) return (int)e;
    if (hipError_t e = hipMemsetAsync(R.vmax, 0, 4ull * n_slides, st); e != hipSuccess) return (int)e;
    return dt_inten == NYXHIP_U8 ? extrema_and_header<uint8_t>(inten, w, h, n_slides, R, st)
         : dt_inten == NYXHIP_U16 ? extrema_and_header<uint16_t>(inten, w, h, n_slides, R, st)
                                  : extrema_and_header<uint32_t>(inten, w, h, n_slides, R, st);
}

int launch_slide_clouds(const void* inten, int dt_inten, uint32_t w, uint32_t h, uint32_t first, uint32_t n_slides, uint16_t* cx, uint16_t* cy, uint32_t* cv, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    return dt_inten == NYXHIP_U8 ? clouds<uint8_t>(inten, w, h, first, n_slides, cx, cy, cv, st)
         : dt_inten == NYXHIP_U16 ? clouds<uint16_t>(inten, w, h, first, n_slides, cx, cy, cv, st)
                                  : clouds<uint32_t>(inten, w, h, first, n_slides, cx, cy, cv, st);
}

} // namespace nyxhip
