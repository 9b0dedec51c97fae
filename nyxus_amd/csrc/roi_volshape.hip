// roi_volshape.hip -- the volume shape unit: the 14 shape codes of the reference's Feature3D enum (D3_SurfaceFeature,
// features/3d_surface.cpp:322-516) from the voxel clouds of a batch of volumes, four launches per chunk of ROIs.
//
//   0 vsh_scatter_kernel   the cloud into the occupancy box (a byte per cell: a voxel / a voxel of non-zero intensity), per (z, y) row the
//                          smallest and largest x of a voxel of non-zero intensity, and the sums of x, y, z and of their products.  All
//                          sums are 64-bit integers added with atomicAdd: they are exact, so a row's bits do not depend on the order.
//   1 vsh_faces_kernel     the exposed faces: per voxel the 6-neighbours the box does not hold, as an integer.
//   2 vsh_hull_kernel      a workgroup per ROI: per z-plane the two monotone chains over the row extremes (the hull vertices of the plane:
//                          every vertex of the 3-D hull is one of them), compacted into the candidate list; then 6 V of the hull by
//                          gift wrapping with exact integer predicates (below).
//   3 vsh_close_kernel     a lane per ROI: the covariance from the integer sums, its eigenvalues by cyclic Jacobi, the 14 columns.
//
// THE HULL.  The served value is the exact volume of the convex hull of the centres of the voxels of non-zero
// intensity, 0 where they span fewer than three dimensions; the reference's float quickhull is not exact.  orient3d of box-relative
// 16-bit coordinates is below 6 * 2^48 and is evaluated in int64.  From a directed hull edge (a, b) the pivot c is the candidate every
// other candidate lies on the non-negative side of; every candidate with orient3d(a, b, c, .) == 0 lies on that facet, whose boundary is
// walked as a polygon: from v the next vertex is the candidate of the plane that has all others on its left, the turn decided as
// orient3d against a candidate q off the plane, collinear ties to the farthest.  Every boundary edge is marked in the visited set and its
// twin pushed; the facet adds det(a0, u, v) per boundary edge (u, v), a fan from its first vertex against the box origin.  The sum is
// -6 V as an integer: it does not depend on the order of the candidates, the facets or the lanes.  Every loop is bounded by the
// candidate count; a bound that is hit, or a twin left unmarked, raises NYXHIP_ERR_INTERNAL.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <math.h>
#include <stdint.h>
#include "launch_util.h"
#include "roi_vol.h"
#include "roi_volshape.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

typedef unsigned long long u64;
typedef long long i64;

struct VsRoi {
    uint64_t roi, off, n64;
    uint32_t w, h, d;
    uint64_t cells;
};
__device__ __forceinline__ VsRoi vs_roi(const VolshapeArgs& A, uint32_t j)
{
    VsRoi R;
    R.roi = A.roi0 + j;
    R.off = A.px_offset[R.roi];
    R.n64 = A.px_offset[R.roi + 1] - R.off;
    R.w = A.bbox_w[R.roi]; R.h = A.bbox_h[R.roi]; R.d = A.bbox_d[R.roi];
    const bool sides = R.w <= kVolMaxSide && R.h <= kVolMaxSide && R.d <= kVolMaxSide;
    R.cells = sides ? (uint64_t)R.w * R.h * R.d : ~0ull;
    return R;
}
// what the kernels touch: an ROI with voxels inside what the strides were sized for (vsh_scatter_kernel raises the status of the others)
__device__ __forceinline__ bool vs_fits(const VolshapeArgs& A, const VsRoi& R)
{
    return R.cells != 0 && R.cells <= (uint64_t)A.max_cells && R.cells <= (uint64_t)kVolMaxCells && R.n64 <= (uint64_t)kVolMaxCells && R.w <= A.side_max[0] &&
           R.h <= A.side_max[1] && R.d <= A.side_max[2] && (uint64_t)R.h * R.d <= (uint64_t)A.rows_max;
}

__device__ __forceinline__ u64 wave_sum(u64 v)
{
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
    return v;
}

// ---- 0: occupancy, row extremes, moments ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vsh_scatter_kernel(const VolshapeArgs A)
{
    const int tid = threadIdx.x;
    const VsRoi R = vs_roi(A, blockIdx.y);
    if (R.n64 == 0) return;
    const bool first = tid == 0 && blockIdx.x == 0;
    if (R.cells == 0) { if (first) atomicCAS(A.status, 0, NYXHIP_ERR_INVALID_ARG); return; }   // voxels, and no box to hold them
    if (!vs_fits(A, R)) { if (first) atomicCAS(A.status, 0, NYXHIP_ERR_ROI_TOO_LARGE); return; }
    unsigned char* const occ = A.occ + (uint64_t)blockIdx.y * A.occ_stride;
    uint32_t* const lo = A.row_lo + (uint64_t)blockIdx.y * A.row_stride;
    uint32_t* const hi = A.row_hi + (uint64_t)blockIdx.y * A.row_stride;
    u64 s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + (uint64_t)tid; i < R.n64; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t x = A.x[R.off + i], y = A.y[R.off + i], z = A.z[R.off + i];
        if (x >= R.w || y >= R.h || z >= R.d) { atomicCAS(A.status, 0, NYXHIP_ERR_INVALID_ARG); continue; }   // never stored
        const bool lit = A.inten[R.off + i] != 0u;
        const uint32_t row = z * R.h + y;
        occ[(uint64_t)row * R.w + x] = lit ? 3 : 1;
        if (lit) { atomicMax(&lo[row], 65536u - x); atomicMax(&hi[row], x + 1u); }
        s[0] += x; s[1] += y; s[2] += z;
        s[3] += (u64)x * x; s[4] += (u64)y * y; s[5] += (u64)z * z;
        s[6] += (u64)x * y; s[7] += (u64)x * z; s[8] += (u64)y * z;
    }
    u64* const head = A.head + (uint64_t)blockIdx.y * kVshHead;
    for (int k = 0; k < 9; k++) {
        const u64 v = wave_sum(s[k]);
        if ((tid & 63) == 0 && v) atomicAdd(&head[VSH_H_SUM + k], v);
    }
}

// ---- 1: exposed faces -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vsh_faces_kernel(const VolshapeArgs A)
{
    const int tid = threadIdx.x;
    const VsRoi R = vs_roi(A, blockIdx.y);
    if (R.n64 == 0 || !vs_fits(A, R)) return;
    const unsigned char* const occ = A.occ + (uint64_t)blockIdx.y * A.occ_stride;
    const uint64_t wh = (uint64_t)R.w * R.h;
    u64 faces = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + (uint64_t)tid; i < R.n64; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t x = A.x[R.off + i], y = A.y[R.off + i], z = A.z[R.off + i];
        if (x >= R.w || y >= R.h || z >= R.d) continue;
        const uint64_t c = ((uint64_t)z * R.h + y) * R.w + x;
        faces += (x == 0u || !occ[c - 1u]) + (x + 1u == R.w || !occ[c + 1u]) + (y == 0u || !occ[c - R.w]) + (y + 1u == R.h || !occ[c + R.w]) +
                 (z == 0u || !occ[c - wh]) + (z + 1u == R.d || !occ[c + wh]);
    }
    faces = wave_sum(faces);
    if ((tid & 63) == 0 && faces) atomicAdd(&A.head[(uint64_t)blockIdx.y * kVshHead + VSH_H_FACES], faces);
}

// ---- 2: the hull ------------------------------------------------------------------------------------------------------------------
struct P3 { i64 x, y, z; };
__device__ __forceinline__ P3 vs_point(u64 k) { return {(i64)(k >> 32), (i64)((k >> 16) & 0xFFFFu), (i64)(k & 0xFFFFu)}; }
// det(b - a, c - a, d - a): positive when d lies on the side of the plane (a, b, c) its normal (b - a) x (c - a) points to
__device__ __forceinline__ i64 orient3d(const P3& a, const P3& b, const P3& c, const P3& d)
{
    const i64 bx = b.x - a.x, by = b.y - a.y, bz = b.z - a.z, cx = c.x - a.x, cy = c.y - a.y, cz = c.z - a.z, dx = d.x - a.x, dy = d.y - a.y, dz = d.z - a.z;
    return bx * (cy * dz - cz * dy) - by * (cx * dz - cz * dx) + bz * (cx * dy - cy * dx);
}
__device__ __forceinline__ bool collinear(const P3& a, const P3& b, const P3& d)
{
    const i64 bx = b.x - a.x, by = b.y - a.y, bz = b.z - a.z, dx = d.x - a.x, dy = d.y - a.y, dz = d.z - a.z;
    return by * dz - bz * dy == 0 && bz * dx - bx * dz == 0 && bx * dy - by * dx == 0;
}
__device__ __forceinline__ i64 dist2(const P3& a, const P3& b) { return (b.x - a.x) * (b.x - a.x) + (b.y - a.y) * (b.y - a.y) + (b.z - a.z) * (b.z - a.z); }

// The winner among the candidates [0, C) that pass `ok`, by the comparator `beats(m, o)`: o replaces m.  Every lane takes a stride of
// the candidates, the lanes of a wave meet by shuffles, and every lane folds the four wave winners from `red` (LDS) in the same order.
// -1: no candidate passes.  All lanes return the winner.
template <class Ok, class Beats>
__device__ __forceinline__ int tournament(uint32_t C, int* red, Ok ok, Beats beats)
{
    const int tid = threadIdx.x;
    int best = -1;
    for (uint32_t i = tid; i < C; i += 256u)
        if (ok((int)i) && (best < 0 || beats(best, (int)i))) best = (int)i;
    for (int s = 32; s > 0; s >>= 1) {
        const int o = __shfl_down(best, s, 64);            // (a lane past the wave's end reads its own winner, which never beats itself)
        if (o >= 0 && (best < 0 || beats(best, o))) best = o;
    }
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    int r = red[0];
    for (int w = 1; w < 4; w++) {
        const int o = red[w];
        if (o >= 0 && (r < 0 || beats(r, o))) r = o;
    }
    __syncthreads();
    return r;
}

// the visited set: directed edges (u, v) of candidate indices as keys (u << 32 | v) + 1 in an open-addressed table of T (a power of two)
// words; lane 0 alone touches it
__device__ __forceinline__ u64 vs_key(int u, int v) { return (((u64)(uint32_t)u << 32) | (uint32_t)v) + 1u; }
__device__ __forceinline__ uint64_t vs_slot(u64 key, uint64_t T) { return (uint64_t)((key * 0x9E3779B97F4A7C15ull) >> 20) & (T - 1u); }
__device__ __forceinline__ bool vs_seen(const u64* tab, uint64_t T, u64 key)
{
    for (uint64_t p = vs_slot(key, T), n = 0; n < T; n++, p = (p + 1u) & (T - 1u)) {
        if (tab[p] == key) return true;
        if (tab[p] == 0) return false;
    }
    return false;
}
__device__ __forceinline__ void vs_mark(u64* tab, uint64_t T, u64 key)
{
    for (uint64_t p = vs_slot(key, T), n = 0; n < T; n++, p = (p + 1u) & (T - 1u)) {
        if (tab[p] == key) return;
        if (tab[p] == 0) { tab[p] = key; return; }
    }
}

// LDS of vsh_hull_kernel: the tournament's tree, the words lane 0 hands to the workgroup, then the candidates, the visited set and
// the edge stack of an ROI of up to kVshLdsCand candidates
__host__ __device__ inline uint32_t vsh_hull_lds(uint32_t lds_cand) { return 1024u + 64u + vsh_lds_bytes(lds_cand); }

__global__ __launch_bounds__(256) void vsh_hull_kernel(const VolshapeArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    int* const red = (int*)lds_raw;                        // the winners of the four waves
    int* const sh = (int*)(lds_raw + 1024);                // [0] candidate count, [1] an edge was popped, [2] [3] the edge, [4] raise
    const int tid = threadIdx.x;
    const VsRoi R = vs_roi(A, blockIdx.x);
    if (R.n64 == 0 || !vs_fits(A, R)) return;
    u64* const head = A.head + (uint64_t)blockIdx.x * kVshHead;
    const uint32_t* const lo = A.row_lo + (uint64_t)blockIdx.x * A.row_stride;
    const uint32_t* const hi = A.row_hi + (uint64_t)blockIdx.x * A.row_stride;
    uint32_t* const chain = A.chain + (uint64_t)blockIdx.x * 2u * A.row_stride;
    u64* const gcand = A.cand + (uint64_t)blockIdx.x * A.cand_stride;

    // the candidates: a lane per plane runs the two chains over the plane's row extremes, which come sorted by y.  Going up, the left
    // chain (smallest x per row) keeps right turns only and the right chain (largest x) left turns only: what stays are the vertices
    // of the plane's 2-D hull.  A point both chains end in (a row of one voxel at the bottom or the top) is listed once.
    if (tid == 0) sh[0] = 0;
    __syncthreads();
    for (uint32_t z = tid; z < R.d; z += 256u) {
        uint32_t* const L = chain + (uint64_t)z * 2u * R.h;
        uint32_t* const Rt = L + R.h;
        uint32_t nl = 0, nr = 0;
        for (uint32_t y = 0; y < R.h; y++) {
            const uint32_t row = z * R.h + y;
            if (hi[row] == 0u) continue;
            const i64 xl = (i64)(65536u - lo[row]), xr = (i64)(hi[row] - 1u);
            while (nl >= 2u) {
                const i64 ox = L[nl - 2u] & 0xFFFFu, oy = L[nl - 2u] >> 16, ax = L[nl - 1u] & 0xFFFFu, ay = L[nl - 1u] >> 16;
                if ((ax - ox) * ((i64)y - oy) - (ay - oy) * (xl - ox) >= 0) nl--; else break;
            }
            L[nl++] = (uint32_t)xl | (y << 16);
            while (nr >= 2u) {
                const i64 ox = Rt[nr - 2u] & 0xFFFFu, oy = Rt[nr - 2u] >> 16, ax = Rt[nr - 1u] & 0xFFFFu, ay = Rt[nr - 1u] >> 16;
                if ((ax - ox) * ((i64)y - oy) - (ay - oy) * (xr - ox) <= 0) nr--; else break;
            }
            Rt[nr++] = (uint32_t)xr | (y << 16);
        }
        if (nl == 0u) continue;
        // (the right chain's ends repeat the left chain's where the bottom or the top row holds one point)
        const uint32_t r0 = Rt[0] == L[0] ? 1u : 0u, r1 = (nr > r0 && Rt[nr - 1u] == L[nl - 1u] && (nl > 1u || r0 == 0u)) ? nr - 1u : nr;
        const uint32_t n = nl + (r1 > r0 ? r1 - r0 : 0u);
        const uint32_t at = (uint32_t)atomicAdd(&sh[0], (int)n);
        uint32_t k = at;
        for (uint32_t i = 0; i < nl; i++) gcand[k++] = ((u64)(L[i] & 0xFFFFu) << 32) | ((u64)(L[i] >> 16) << 16) | z;
        for (uint32_t i = r0; i < r1; i++) gcand[k++] = ((u64)(Rt[i] & 0xFFFFu) << 32) | ((u64)(Rt[i] >> 16) << 16) | z;
    }
    __syncthreads();
    const uint32_t C = (uint32_t)sh[0];
    __syncthreads();
    if (tid == 0) head[VSH_H_NCAND] = C;
    if (C < 4u) return;                                    // (6 V stays 0: fewer than four points span no volume)
    if ((uint64_t)C > A.cand_stride) { if (tid == 0) atomicCAS(A.status, 0, NYXHIP_ERR_INTERNAL); return; }

    // one code path, two storage bases
    const bool in_lds = C <= A.lds_cand;                   // (lds_cand is kVshLdsCand unless no ROI of the launch can reach it)
    u64* const cand = in_lds ? (u64*)(lds_raw + 1088) : gcand;
    u64* const tab = in_lds ? (u64*)(lds_raw + 1088 + 8u * A.lds_cand) : A.visited + (uint64_t)blockIdx.x * A.visited_stride;
    u64* const stack = in_lds ? (u64*)(lds_raw + 1088 + 8u * A.lds_cand + 8u * (uint32_t)vsh_table(A.lds_cand)) : A.stack + (uint64_t)blockIdx.x * A.stack_stride;
    const uint64_t T = vsh_table(C), stack_cap = 3ull * C;
    if (in_lds)
        for (uint32_t i = tid; i < C; i += 256u) cand[i] = gcand[i];
    for (uint64_t i = tid; i < T; i += 256u) tab[i] = 0;
    __syncthreads();
    auto P = [&](int i) { return vs_point(cand[i]); };

    // the first edge.  a: the smallest candidate by (x, y, z), a vertex.  Pivot the plane through a and a + ez about that axis until all
    // candidates lie on one side (c1), then take a's neighbour on the 2-D hull of the candidates of that plane: (a, b) is a hull edge.
    const int a0 = tournament(C, red, [&](int) { return true; }, [&](int m, int o) { return cand[o] < cand[m]; });
    const P3 pa = P(a0), pz = {pa.x, pa.y, pa.z + 1};
    const int c1 = tournament(C, red, [&](int i) { const P3 p = P(i); return p.x != pa.x || p.y != pa.y; },
                              [&](int m, int o) { return orient3d(pa, pz, P(m), P(o)) < 0; });
    if (c1 < 0) return;                                    // a line along z
    const P3 pc1 = P(c1);
    const int q1 = tournament(C, red, [&](int i) { return orient3d(pa, pz, pc1, P(i)) != 0; }, [&](int, int) { return false; });
    if (q1 < 0) return;                                    // a plane
    const P3 pq1 = P(q1);
    const int b0 = tournament(C, red, [&](int i) { return i != a0 && orient3d(pa, pz, pc1, P(i)) == 0; },
                              [&](int m, int o) {
                                  const i64 t = orient3d(pa, P(m), P(o), pq1);
                                  return t < 0 || (t == 0 && dist2(pa, P(o)) > dist2(pa, P(m)));
                              });
    if (b0 < 0) { if (tid == 0) atomicCAS(A.status, 0, NYXHIP_ERR_INTERNAL); return; }

    // lane 0 keeps the stack, the visited set and the sum
    uint64_t sp = 0, marked = 0;
    i64 unmatched = 0;
    u64 acc = 0;
    bool flat = false;
    if (tid == 0) { stack[sp++] = vs_key(a0, b0); stack[sp++] = vs_key(b0, a0); sh[4] = 0; }
    __syncthreads();
    for (uint64_t facets = 0;; facets++) {
        if (tid == 0) {
            sh[1] = 0;
            while (sp > 0) {
                const u64 e = stack[--sp];
                if (!vs_seen(tab, T, e)) { sh[1] = 1; sh[2] = (int)((e - 1u) >> 32); sh[3] = (int)((e - 1u) & 0xFFFFFFFFu); break; }
            }
            if (sh[1] && facets >= 2ull * C) { sh[1] = 0; sh[4] = 1; }   // a hull of C vertices has at most 2 C - 4 facets
        }
        __syncthreads();
        if (!sh[1]) break;
        const int a = sh[2], b = sh[3];
        const P3 fa = P(a), fb = P(b);
        const int c = tournament(C, red, [&](int i) { return !collinear(fa, fb, P(i)); }, [&](int m, int o) { return orient3d(fa, fb, P(m), P(o)) < 0; });
        if (c < 0) { flat = true; break; }                 // a line
        const P3 fc = P(c);
        // q: a candidate off the plane; one on its negative side would mean the pivot is no supporting plane
        const int q = tournament(C, red, [&](int i) { return orient3d(fa, fb, fc, P(i)) != 0; }, [&](int m, int o) { return orient3d(fa, fb, fc, P(o)) < 0; });
        if (q < 0) { flat = true; break; }                 // a plane
        const P3 fq = P(q);
        if (orient3d(fa, fb, fc, fq) < 0) { if (tid == 0) sh[4] = 1; break; }
        int u = a, v = b;
        bool bad = false;
        for (uint32_t steps = 0;; steps++) {
            if (tid == 0) {
                const P3 pu = P(u), pv = P(v);
                acc += (u64)(fa.x * (pu.y * pv.z - pu.z * pv.y) - fa.y * (pu.x * pv.z - pu.z * pv.x) + fa.z * (pu.x * pv.y - pu.y * pv.x));
                vs_mark(tab, T, vs_key(u, v));
                marked++;
                if (vs_seen(tab, T, vs_key(v, u))) unmatched--;
                else {
                    unmatched++;
                    if (sp < stack_cap) stack[sp++] = vs_key(v, u); else sh[4] = 1;
                }
                if (marked > 6ull * C) sh[4] = 1;          // at most 3 C - 6 edges, each marked once per direction
            }
            if (v == a) break;
            if (steps >= C) { bad = true; break; }
            const P3 fv = P(v);
            const int w = tournament(C, red, [&](int i) { return i != v && orient3d(fa, fb, fc, P(i)) == 0; },
                                     [&](int m, int o) {
                                         const i64 t = orient3d(fv, P(m), P(o), fq);
                                         return t < 0 || (t == 0 && dist2(fv, P(o)) > dist2(fv, P(m)));
                                     });
            if (w < 0) { bad = true; break; }
            u = v; v = w;
        }
        if (bad) { if (tid == 0) sh[4] = 1; break; }
        __syncthreads();
        if (sh[4]) break;
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) {
        // (a flat cloud is found at the first facet; later no facet of a solid hull lacks its pivot or its q)
        if (sh[4] || (flat && marked != 0) || (!flat && unmatched != 0)) atomicCAS(A.status, 0, NYXHIP_ERR_INTERNAL);
        else if (!flat) head[VSH_H_HULL6V] = (u64)(-(i64)acc);   // the facets are oriented inwards
    }
}

// ---- 3: close ---------------------------------------------------------------------------------------------------------------------
// The eigenvalues of a symmetric 3 x 3 matrix by cyclic Jacobi rotations in fp64, to convergence: a sweep annihilates (0,1), (0,2), (1,2)
// in turn, each by the rotation whose tangent is the smaller root of t^2 + 2 theta t - 1; the sweeps end when the off-diagonal part no
// longer registers against the diagonal.
__device__ void jacobi3(double m[3][3], double ev[3])
{
    for (int sweep = 0; sweep < 64; sweep++) {
        const double off = fabs(m[0][1]) + fabs(m[0][2]) + fabs(m[1][2]);
        const double diag = fabs(m[0][0]) + fabs(m[1][1]) + fabs(m[2][2]);
        if (off == 0.0 || diag + off == diag) break;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                const double apq = m[p][q];
                if (apq == 0.0) continue;
                const double theta = (m[q][q] - m[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                const int r = 3 - p - q;
                const double arp = m[r][p], arq = m[r][q];
                m[p][p] -= t * apq;
                m[q][q] += t * apq;
                m[p][q] = m[q][p] = 0.0;
                m[r][p] = m[p][r] = c * arp - s * arq;
                m[r][q] = m[q][r] = s * arp + c * arq;
            }
    }
    ev[0] = m[0][0]; ev[1] = m[1][1]; ev[2] = m[2][2];
}

__global__ __launch_bounds__(64) void vsh_close_kernel(const VolshapeArgs A)
{
    const uint64_t j = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (j >= A.n_roi) return;
    const VsRoi R = vs_roi(A, (uint32_t)j);
    double* const o = A.out + R.roi * A.ld;
    if (R.n64 == 0) {
        for (int k = 0; k < kVshCols; k++) o[k] = A.soft_nan;
        return;
    }
    if (!vs_fits(A, R)) return;                            // (vsh_scatter_kernel raised the status)
    const u64* const head = A.head + j * kVshHead;
    const double pi = 3.14159265358979323846;
    const double n = (double)R.n64;
    // (the reference adds 4/3 pi / 8 once per voxel, 3d_surface.cpp:357-361; here the product, which differs by the rounding of the sum)
    const double vol = n * (4. / 3. * pi * (1. / 8.)) / 0.5236;
    const double area = (double)head[VSH_H_FACES];
    const double hull = (double)(i64)head[VSH_H_HULL6V] / 6.0;
    o[VSH_AREA] = area;
    o[VSH_AREA_2_VOLUME] = area / vol;
    o[VSH_COMPACTNESS1] = vol / sqrt(pi * area * area * area);
    o[VSH_COMPACTNESS2] = 36. * pi * vol * vol / (area * area * area);
    o[VSH_MESH_VOLUME] = hull;
    o[VSH_SPHERICAL_DISPROPORTION] = area / pow(36. * pi * vol * vol, 1. / 3.);
    o[VSH_SPHERICITY] = pow(36. * pi * vol * vol, 1. / 3.) / area;
    o[VSH_VOLUME_CONVEXHULL] = hull;
    o[VSH_VOXEL_VOLUME] = vol;
    // the covariance with divisor N - 1 from the exact integer sums: N S_ij - S_i S_j is below 2^81, formed in 128 bits and rounded once
    double L[3] = {0.0, 0.0, 0.0};
    if (R.n64 > 1) {
        const u64 N = R.n64;
        const u64* const S = head + VSH_H_SUM;
        const u64* const M = head + VSH_H_MOM;
        const double den = (double)N * (double)(N - 1u);
        auto cov = [&](int mom, int i, int k) { return (double)((__int128)N * (__int128)M[mom] - (__int128)S[i] * (__int128)S[k]) / den; };
        double m[3][3];
        m[0][0] = cov(0, 0, 0); m[1][1] = cov(1, 1, 1); m[2][2] = cov(2, 2, 2);
        m[0][1] = m[1][0] = cov(3, 0, 1); m[0][2] = m[2][0] = cov(4, 0, 2); m[1][2] = m[2][1] = cov(5, 1, 2);
        jacobi3(m, L);
        for (int k = 0; k < 3; k++) if (!(L[k] > 0.0)) L[k] = 0.0;
        if (L[0] < L[1]) { const double t = L[0]; L[0] = L[1]; L[1] = t; }
        if (L[1] < L[2]) { const double t = L[1]; L[1] = L[2]; L[2] = t; }
        if (L[0] < L[1]) { const double t = L[0]; L[0] = L[1]; L[1] = t; }
        // an eigenvalue below 2^-40 of the largest is the rounding of a rank-deficient cloud's zero
        for (int k = 1; k < 3; k++) if (L[k] < L[0] * 0x1p-40) L[k] = 0.0;
    }
    o[VSH_MAJOR_AXIS_LEN] = 4.0 * sqrt(L[0]);
    o[VSH_MINOR_AXIS_LEN] = 4.0 * sqrt(L[1]);
    o[VSH_LEAST_AXIS_LEN] = 4.0 * sqrt(L[2]);
    o[VSH_ELONGATION] = L[0] > 0.0 ? sqrt(L[1] / L[0]) : 0.0;
    o[VSH_FLATNESS] = L[0] > 0.0 ? sqrt(L[2] / L[0]) : 0.0;
}

uint32_t cap_grid(uint64_t n) { return (uint32_t)(n < 1u ? 1u : n > 1024u ? 1024u : n); }

} // namespace

int launch_volshape_step(const VolshapeArgs& a, int step, void* stream)
{
    if (a.n_roi == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nr = (uint32_t)a.n_roi;
    // a workgroup takes 16 voxels per lane, up to 1024 workgroups per ROI
    const dim3 cloud(cap_grid(((uint64_t)a.max_px + 4095u) / 4096u), nr);
    switch (step) {
    case 0: hipLaunchKernelGGL(vsh_scatter_kernel, cloud, dim3(256), 0, st, a); break;
    case 1: hipLaunchKernelGGL(vsh_faces_kernel, cloud, dim3(256), 0, st, a); break;
    case 2: {
        static DeviceOnce optin;                           // (dynamic LDS beyond 64 KiB is an opt-in per kernel)
        if (int orc = optin.run([]() -> int {
                return (int)hipFuncSetAttribute((const void*)vsh_hull_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)vsh_hull_lds(kVshLdsCand));
            }))
            return orc;
        if (a.lds_cand == 0 || a.lds_cand > kVshLdsCand) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(vsh_hull_kernel, dim3(nr), dim3(256), vsh_hull_lds(a.lds_cand), st, a);
        break;
    }
    default: hipLaunchKernelGGL(vsh_close_kernel, dim3((nr + 63u) / 64u), dim3(64), 0, st, a); break;
    }
    return (int)hipGetLastError();
}

int launch_volshape(const VolshapeArgs& a, void* stream)
{
    for (int step = 0; step < kVshSteps; step++)
        if (int rc = launch_volshape_step(a, step, stream)) return rc;
    return 0;
}

} // namespace nyxhip
