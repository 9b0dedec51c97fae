// vol_zone_prims.h -- device helpers the volume zone units share (roi_volzone.hip, roi_voldzone.hip): the bounded union-find chain over
// the cells of a box and the lane-ordered sums of the closing kernels.  Every loop has a bound derived from the box; a loop that reaches
// it raises NYXHIP_ERR_INTERNAL in the status word and leaves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nyxhip.h"

namespace nyxhip {

__device__ __forceinline__ void vz_raise_internal(int* status) { atomicCAS(status, 0, NYXHIP_ERR_INTERNAL); }
__device__ __forceinline__ uint32_t vz_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x.  Labels only decrease along a chase, so it takes fewer than `cells` steps; on the way every visited cell is pointed at
// its grandparent (atomicMin: a label never rises, and stays inside its zone), which keeps the chains short.  `budget` counts the steps
// of one caller: a chase that uses it up raises the error word and leaves.
__device__ __forceinline__ uint32_t vz_find(int* status, uint32_t* Lb, uint32_t x, uint32_t cells, uint32_t& budget)
{
    uint32_t p = vz_ld(&Lb[x]);
    while (p != x) {
        if (budget == 0u || p >= cells) { vz_raise_internal(status); budget = 0u; break; }
        budget--;
        const uint32_t gp = vz_ld(&Lb[p]);
        if (gp >= cells) { vz_raise_internal(status); budget = 0u; break; }
        if (gp != p) atomicMin(&Lb[x], gp);
        x = p;
        p = gp;
    }
    return x;
}
__device__ __forceinline__ void vz_unite(int* status, uint32_t* Lb, uint32_t a, uint32_t b, uint32_t cells)
{
    // a round is repeated only when another thread lowered the root in between; rounds and chase steps share one budget
    uint32_t budget = 4u * cells + 1024u;
    for (;;) {
        a = vz_find(status, Lb, a, cells, budget);
        b = vz_find(status, Lb, b, cells, budget);
        if (a == b || budget == 0u) return;
        budget--;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&Lb[a], b);         // a was a root when its label was still a
        if (old == a) return;
        a = old;
    }
}

// Q sums at once: the 64 per-lane partials of sum q are added in lane order by lane q, and every lane gets the totals
constexpr int kVzSums = 12;
template <int Q> __device__ __forceinline__ void vz_lane_sums(double (&v)[Q], double (*s_p)[64], double* s_r, int lane)
{
    static_assert(Q <= kVzSums, "the LDS of the closing kernels holds kVzSums rows");
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; q++) s_p[q][lane] = v[q];
    __syncthreads();
    if (lane < Q) {
        double t = 0.0;
#pragma unroll 1
        for (int l = 0; l < 64; l++) t += s_p[lane][l];
        s_r[lane] = t;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; q++) v[q] = s_r[q];
}
__device__ __forceinline__ unsigned long long vz_wave_sum_u64(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

} // namespace nyxhip
