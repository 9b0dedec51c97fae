// roi_volzone.hip -- volumes (3-D): the GLRLM and GLSZM blocks of the reference's Feature3D enum (gfx950).
//
// Both classes read a binned box of vol_bin_kernel (roi_vol.hip).  An ROI has ceil(cells / kVzCellsPerWg) workgroups per sweep, each owning
// a fixed range of cells of the ROI's own box; surplus workgroups of the grid leave at once.  No kernel waits for another workgroup: the
// order between the phases is the order of the launches on the stream.
//
//   GLRLM (3d_glrlm.cpp)
//   vz_runs_kernel        (range, ROI, direction): every direction of shifts13 points forward in raster order, so gather_rl_zones yields
//                         the maximal runs of equal non-zero level along it.  A cell whose predecessor is outside the box or of another
//                         level is a run head; it walks its run in the binned box (at most L_k steps, the smallest box side among the
//                         direction's non-zero components) and counts [level][length - 1]: short runs in LDS, merged with integer
//                         atomics, longer ones in the global table directly.  A run that crosses a range boundary is read, not owned.
//   vz_runs_close_kernel  a wave per (ROI, direction): lanes own run lengths j = lane, lane + 64, ..; three passes over the table (sums,
//                         first-order terms, the two variances), per-lane fp64 partials combined in lane order by one lane.
//   vz_runs_ave_kernel    calc_ave over the 13 directional values.
//
//   GLSZM (3d_glszm.cpp): gather_size_zones is a complete depth-first search over 26 neighbours, so a zone is a 26-connected component
//   of equal level; cells of the background level (1 under matlab binning, else 0) are skipped.
//   vz_zone_init_kernel   label = own cell index; background cells get kVzNoLabel; counts zeroed
//   vz_zone_merge_kernel  each cell unites with its 13 raster-earlier neighbours of equal level: union-find, a root links to a smaller
//                         index with atomicMin, so labels only ever decrease; a chase halves the path it walks
//   vz_zone_count_kernel  each cell chases its root (and stores it), then counts itself at the root (a wave adds its lanes of the
//                         leading root in one atomic)
//   vz_zone_emit_kernel   each root: zones up to kVzDenseSizes cells count [level][size - 1] (LDS, merged); larger ones append the key
//                         (size - 1) << 8 | level to the ROI's list in arrival order
//   vz_zone_sort_kernel   a workgroup per ROI: stable LSD radix sort of the list, so no float ever sees the arrival order
//   vz_zone_close_kernel  a wave per ROI: the dense table, then the sorted list compressed to (level, size, count) on the fly
//
// Every chase and every walk has a bound derived from the box (cells, L_k); a loop that reaches it raises NYXHIP_ERR_INTERNAL in the
// status word and leaves.  Everything that more than one thread adds to is an integer.  Nothing of an ROI's row depends on another ROI.
// j * j of the reference is int and overflows above 46340; here it is double(j) * double(j), exact.
// Built with -ffp-contract=off (device_math.h).
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "launch_util.h"
#include "roi_vol.h"
#include "roi_volzone.h"
#include "vol_zone_prims.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

const int kVzShifts[kVzDirs][3] = {{1, 1, 1}, {1, 1, 0}, {1, 1, -1}, {1, 0, 1}, {1, 0, 0}, {1, 0, -1}, {1, -1, 1},
                                   {1, -1, 0}, {1, -1, -1}, {0, 1, 1}, {0, 1, 0}, {0, 1, -1}, {0, 0, 1}};

namespace {

// shifts13[] of 3d_glrlm.cpp:17-32: (dz, dy, dx)
__constant__ int c_vz_shift[kVzDirs][3] = {{1, 1, 1}, {1, 1, 0}, {1, 1, -1}, {1, 0, 1}, {1, 0, 0}, {1, 0, -1}, {1, -1, 1},
                                           {1, -1, 0}, {1, -1, -1}, {0, 1, 1}, {0, 1, 0}, {0, 1, -1}, {0, 0, 1}};

struct VzRoi {
    uint64_t roi, off, n64;
    uint32_t w, h, d, vmin, vmax;
    uint64_t cells;
};
__device__ __forceinline__ VzRoi vz_roi(const VolzoneArgs& A, uint32_t j)
{
    VzRoi R;
    R.roi = A.roi0 + j;
    R.off = A.px_offset[R.roi];
    R.n64 = A.px_offset[R.roi + 1] - R.off;
    R.w = A.bbox_w[R.roi]; R.h = A.bbox_h[R.roi]; R.d = A.bbox_d[R.roi];
    R.vmin = A.vmin[R.roi]; R.vmax = A.vmax[R.roi];
    const bool sides = R.w <= kVolMaxSide && R.h <= kVolMaxSide && R.d <= kVolMaxSide;
    R.cells = sides ? (uint64_t)R.w * R.h * R.d : ~0ull;
    return R;
}
// what the sweeps touch: an ROI with voxels that is not flat, inside what the strides were sized for (vol_bin_kernel raises the status
// of the others)
__device__ __forceinline__ bool vz_swept(const VolzoneArgs& A, const VzRoi& R)
{
    return R.n64 != 0 && R.cells != 0 && R.cells <= (uint64_t)A.max_cells && R.cells <= (uint64_t)kVolMaxCells && R.vmin != R.vmax &&
           R.w <= A.side_max[0] && R.h <= A.side_max[1] && R.d <= A.side_max[2];
}
__device__ __forceinline__ void vz_internal(const VolzoneArgs& A) { atomicCAS(A.status, 0, NYXHIP_ERR_INTERNAL); }

// ---- GLRLM ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vz_runs_kernel(const VolzoneArgs A)
{
    __shared__ uint32_t s_T[(kVzLevelCap + 1) * kVzShortRuns];
    __shared__ uint32_t s_max;
    const int tid = threadIdx.x;
    const VzRoi R = vz_roi(A, blockIdx.y);
    if (!vz_swept(A, R)) return;
    const uint32_t cells = (uint32_t)R.cells;
    if ((uint64_t)blockIdx.x * kVzCellsPerWg >= (uint64_t)cells) return;
    const uint32_t c0 = blockIdx.x * kVzCellsPerWg, c1 = cells - c0 > kVzCellsPerWg ? c0 + kVzCellsPerWg : cells;
    const uint32_t k = blockIdx.z, rows = A.rows[VZ_GLRLM];
    const int dz = c_vz_shift[k][0], dy = c_vz_shift[k][1], dx = c_vz_shift[k][2];
    const uint32_t L = vz_dir_len(dz, dy, dx, R.w, R.h, R.d);
    for (uint32_t i = tid; i < rows * kVzShortRuns; i += 256u) s_T[i] = 0u;
    if (tid == 0) s_max = 0u;
    __syncthreads();
    const unsigned char* const D = A.box[VZ_GLRLM] + (uint64_t)blockIdx.y * A.box_stride;
    uint32_t* const H = A.rl_tab + (uint64_t)blockIdx.y * A.rl_stride;
    uint32_t* const G = H + A.rl_dir_off[k];
    const int w = (int)R.w, h = (int)R.h, d = (int)R.d;
    const uint32_t wh = R.w * R.h;
    const int step = (dz * h + dy) * w + dx;               // the direction in cells of the box (positive: it points forward)
    uint32_t longest = 0;
    for (uint32_t i = c0 + (uint32_t)tid; i < c1; i += 256u) {
        const uint32_t c = D[i];
        if (c == 0u || c >= rows) continue;                // level 0 is blank (3d_glrlm.cpp:57); (no level reaches `rows`: the binning kernel)
        const uint32_t uz = i / wh, rem = i - uz * wh, uy = rem / R.w;
        const int z = (int)uz, y = (int)uy, x = (int)(rem - uy * R.w);
        const int pz = z - dz, py = y - dy, px = x - dx;
        if (pz >= 0 && py >= 0 && py < h && px >= 0 && px < w && D[(int)i - step] == c) continue;   // not a head
        uint32_t len = 1;
        for (;; len++) {                                   // at most L cells lie on the line inside the box
            const int nz = z + (int)len * dz, ny = y + (int)len * dy, nx = x + (int)len * dx;
            if (nz >= d || ny < 0 || ny >= h || nx < 0 || nx >= w) break;
            if (len >= L) { vz_internal(A); break; }
            if (D[(int)i + (int)len * step] != c) break;
        }
        if (len <= kVzShortRuns) atomicAdd(&s_T[c * kVzShortRuns + (len - 1u)], 1u);
        else atomicAdd(&G[(uint64_t)c * L + (len - 1u)], 1u);
        longest = len > longest ? len : longest;
    }
    if (longest) atomicMax(&s_max, longest);
    __syncthreads();
    for (uint32_t i = tid; i < rows * kVzShortRuns; i += 256u) {
        const uint32_t v = s_T[i];
        if (v == 0u) continue;
        const uint32_t c = i / kVzShortRuns, j = i - c * kVzShortRuns;   // (j < L: a run of that length was met)
        atomicAdd(&G[(uint64_t)c * L + j], v);
    }
    if (tid == 0 && s_max) atomicMax(&H[k], s_max);
}

// 3d_glrlm.cpp:224-259 and the calc_* functions below it.  The matrix P is [Ng x Nr]; rows of absent levels and columns beyond the
// longest run are empty and add exactly 0 to every sum (the entropy term too: 0 * log2(EPS)), so the loops run over the table rows.
__global__ __launch_bounds__(64) void vz_runs_close_kernel(const VolzoneArgs A)
{
    __shared__ uint32_t s_row[kVzLevelCap + 1];
    __shared__ double s_p[kVzSums][64];
    __shared__ double s_r[kVzSums];
    const int lane = threadIdx.x;
    const uint32_t k = blockIdx.x, rows = A.rows[VZ_GLRLM];
    const VzRoi R = vz_roi(A, blockIdx.y);
    double* const o = A.out + R.roi * A.ld + A.col[VZ_GLRLM] + k;      // code c at o[c * 13]
    if (R.n64 == 0 || (R.vmin == R.vmax && R.cells != 0)) {            // no voxels; a flat ROI (3d_glrlm.cpp:115-136)
        if (lane < kVzGlrlmCodes) o[lane * kVzDirs] = A.soft_nan;
        return;
    }
    if (!vz_swept(A, R)) return;                           // (the binning kernel raised the status)
    const int dz = c_vz_shift[k][0], dy = c_vz_shift[k][1], dx = c_vz_shift[k][2];
    const uint32_t L = vz_dir_len(dz, dy, dx, R.w, R.h, R.d);
    const uint32_t* const H = A.rl_tab + (uint64_t)blockIdx.y * A.rl_stride;
    const uint32_t* const G = H + A.rl_dir_off[k];
    uint32_t Nr = H[k];
    if (Nr > L) { if (lane == 0) vz_internal(A); Nr = L; }
    for (uint32_t i = lane; i < rows; i += 64u) s_row[i] = 0u;
    __syncthreads();
    // pass 1: the column sums rj (3d_glrlm.cpp:336-343), the row sums, the total
    unsigned long long tot = 0, sq = 0;
    double a1[1] = {0.0};                                  // SRE: sum over j of rj / j^2
    for (uint32_t j = lane; j < Nr; j += 64u) {
        uint32_t cs = 0;
        for (uint32_t i = 1; i < rows; i++) {
            const uint32_t p = G[(uint64_t)i * L + j];
            if (p) { cs += p; atomicAdd(&s_row[i], p); }
        }
        tot += cs;
        sq += (unsigned long long)cs * cs;
        const double jj = (double)(j + 1u);
        a1[0] += (double)cs / (jj * jj);
    }
    tot = vz_wave_sum_u64(tot);
    sq = vz_wave_sum_u64(sq);
    vz_lane_sums(a1, s_p, s_r, lane);
    const double sre = a1[0];
    if (tot == 0ull) {                                     // every formula answers 0 for an empty matrix; RP = 0 / Np
        if (lane < kVzGlrlmCodes) o[lane * kVzDirs] = 0.0;
        return;
    }
    const double sum = (double)tot;
    // pass 2: the term-by-term sums
    enum { LRE, MUG, MUR, RE, LGL, HGL, SRL, SRH, LRL, LRH, N2 };
    double a2[N2] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t j = lane; j < Nr; j += 64u) {
        const double jj = (double)(j + 1u), j2 = jj * jj;
        for (uint32_t i = 1; i < rows; i++) {
            const uint32_t pi = G[(uint64_t)i * L + j];
            if (pi == 0u) continue;
            const double p = (double)(int)pi, inten = (double)i, i2 = inten * inten;
            a2[LRE] += p * j2;
            a2[MUG] += p / sum * inten;
            a2[MUR] += p / sum * jj;
            a2[RE] += p / sum * (fast_log10(p / sum + 2.2e-16) / 0.30102999566);
            a2[LGL] += p / i2;
            a2[HGL] += p * inten * inten;
            a2[SRL] += p / (i2 * j2);
            a2[SRH] += p * i2 / j2;
            a2[LRL] += p * j2 / i2;
            a2[LRH] += p * (i2 * j2);
        }
    }
    vz_lane_sums(a2, s_p, s_r, lane);
    const double lre = a2[LRE], muG = a2[MUG], muR = a2[MUR], re = a2[RE], lgl = a2[LGL], hgl = a2[HGL], srl = a2[SRL], srh = a2[SRH], lrl = a2[LRL], lrh = a2[LRH];
    // pass 3: the variances about the two means
    double a3[2] = {0.0, 0.0};
    for (uint32_t j = lane; j < Nr; j += 64u) {
        const double jj = (double)(j + 1u);
        for (uint32_t i = 1; i < rows; i++) {
            const uint32_t pi = G[(uint64_t)i * L + j];
            if (pi == 0u) continue;
            const double p = (double)(int)pi, inten = (double)i;
            a3[0] += p / sum * ((inten - muG) * (inten - muG));
            a3[1] += p / sum * ((jj - muR) * (jj - muR));
        }
    }
    vz_lane_sums(a3, s_p, s_r, lane);
    const double glv = a3[0], rv = a3[1];
    if (lane != 0) return;
    double gln = 0.0;
#pragma unroll 1
    for (uint32_t i = 1; i < rows; i++) { const double s = (double)s_row[i]; gln += s * s; }
    const double rln = (double)sq;                         // exact: at most (2^24)^2
    o[0 * kVzDirs] = sre / sum;
    o[1 * kVzDirs] = lre / sum;
    o[2 * kVzDirs] = gln / sum;
    o[3 * kVzDirs] = gln / (sum * sum);
    o[4 * kVzDirs] = rln / sum;
    o[5 * kVzDirs] = rln / (sum * sum);
    o[6 * kVzDirs] = sum / (double)R.n64;
    o[7 * kVzDirs] = glv;
    o[8 * kVzDirs] = rv;
    o[9 * kVzDirs] = -re;
    o[10 * kVzDirs] = lgl / sum;
    o[11 * kVzDirs] = hgl / sum;
    o[12 * kVzDirs] = srl / sum;
    o[13 * kVzDirs] = srh / sum;
    o[14 * kVzDirs] = lrl / sum;
    o[15 * kVzDirs] = lrh / sum;
}

// calc_ave (texture_feature.h:121-130): std::reduce(begin, end) / 13 in libstdc++'s order, as vol_glcm_ave_kernel keeps it.  soft_nan
// values are averaged like any other.
__global__ __launch_bounds__(256) void vz_runs_ave_kernel(const VolzoneArgs A)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= A.n_roi * (uint64_t)kVzGlrlmCodes) return;
    const uint32_t j = (uint32_t)(t / kVzGlrlmCodes), c = (uint32_t)(t - (uint64_t)j * kVzGlrlmCodes);
    const VzRoi R = vz_roi(A, j);
    const bool blank = R.n64 == 0 || (R.vmin == R.vmax && R.cells != 0);
    if (!blank && !vz_swept(A, R)) return;
    double* const orow = A.out + R.roi * A.ld + A.col[VZ_GLRLM];
    const double* const v = orow + c * kVzDirs;
    double init = 0.0;
    init = init + ((v[0] + v[1]) + (v[2] + v[3]));
    init = init + ((v[4] + v[5]) + (v[6] + v[7]));
    init = init + ((v[8] + v[9]) + (v[10] + v[11]));
    init = init + v[12];
    orow[kVzGlrlmCodes * kVzDirs + c] = init / 13.0;
}

// ---- GLSZM ------------------------------------------------------------------------------------------------------------------------
struct VzRange { uint32_t cells, c0, c1; bool any; };
__device__ __forceinline__ VzRange vz_range(const VolzoneArgs& A, const VzRoi& R)
{
    VzRange g{0u, 0u, 0u, false};
    if (!vz_swept(A, R)) return g;
    g.cells = (uint32_t)R.cells;
    if ((uint64_t)blockIdx.x * kVzCellsPerWg >= (uint64_t)g.cells) return g;
    g.c0 = blockIdx.x * kVzCellsPerWg;
    g.c1 = g.cells - g.c0 > kVzCellsPerWg ? g.c0 + kVzCellsPerWg : g.cells;
    g.any = true;
    return g;
}

__global__ __launch_bounds__(256) void vz_zone_init_kernel(const VolzoneArgs A)
{
    const VzRoi R = vz_roi(A, blockIdx.y);
    const VzRange g = vz_range(A, R);
    if (!g.any) return;
    const unsigned char* const D = A.box[VZ_GLSZM] + (uint64_t)blockIdx.y * A.box_stride;
    uint32_t* const Lb = A.sz_label + (uint64_t)blockIdx.y * A.cell_stride;
    uint32_t* const Cn = A.sz_count + (uint64_t)blockIdx.y * A.cell_stride;
    const uint32_t zeroI = A.g[VZ_GLSZM] > 0 ? 1u : 0u;    // 3d_glszm.cpp:517
    for (uint32_t i = g.c0 + threadIdx.x; i < g.c1; i += 256u) {
        Lb[i] = D[i] == zeroI ? kVzNoLabel : i;
        Cn[i] = 0u;
    }
}

__global__ __launch_bounds__(256) void vz_zone_merge_kernel(const VolzoneArgs A)
{
    const VzRoi R = vz_roi(A, blockIdx.y);
    const VzRange g = vz_range(A, R);
    if (!g.any) return;
    const unsigned char* const D = A.box[VZ_GLSZM] + (uint64_t)blockIdx.y * A.box_stride;
    uint32_t* const Lb = A.sz_label + (uint64_t)blockIdx.y * A.cell_stride;
    const uint32_t zeroI = A.g[VZ_GLSZM] > 0 ? 1u : 0u;
    const int w = (int)R.w, h = (int)R.h;
    const uint32_t wh = R.w * R.h;
    for (uint32_t i = g.c0 + threadIdx.x; i < g.c1; i += 256u) {
        const uint32_t c = D[i];
        if (c == zeroI) continue;
        const uint32_t uz = i / wh, rem = i - uz * wh, uy = rem / R.w;
        const int z = (int)uz, y = (int)uy, x = (int)(rem - uy * R.w);
        // the 13 neighbours that come earlier in raster order: the 9 of the slice below, the 3 of the row above, the cell to the left
        for (int dz = -1; dz <= 0; dz++) {
            const int nz = z + dz;
            if (nz < 0) continue;
            for (int dy = -1; dy <= (dz < 0 ? 1 : 0); dy++) {
                const int ny = y + dy;
                if (ny < 0 || ny >= h) continue;
                for (int dx = -1; dx <= ((dz < 0 || dy < 0) ? 1 : -1); dx++) {
                    const int nx = x + dx;
                    if (nx < 0 || nx >= w) continue;
                    const uint32_t n = ((uint32_t)nz * R.h + (uint32_t)ny) * R.w + (uint32_t)nx;
                    if (D[n] == c) vz_unite(A.status, Lb, i, n, g.cells);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void vz_zone_count_kernel(const VolzoneArgs A)
{
    const VzRoi R = vz_roi(A, blockIdx.y);
    const VzRange g = vz_range(A, R);
    if (!g.any) return;
    uint32_t* const Lb = A.sz_label + (uint64_t)blockIdx.y * A.cell_stride;
    uint32_t* const Cn = A.sz_count + (uint64_t)blockIdx.y * A.cell_stride;
    const int lane = threadIdx.x & 63;
    for (uint32_t i0 = g.c0; i0 < g.c1; i0 += 256u) {      // (the trip count is the workgroup's: every lane reaches the ballots)
        const uint32_t i = i0 + threadIdx.x;
        uint32_t r = kVzNoLabel;
        if (i < g.c1 && vz_ld(&Lb[i]) != kVzNoLabel) {
            uint32_t budget = g.cells;
            r = vz_find(A.status, Lb, i, g.cells, budget);
            __hip_atomic_store(&Lb[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a root keeps its own index)
        }
        const unsigned long long have = __ballot(r != kVzNoLabel);
        if (have == 0ull) continue;
        const uint32_t lead = (uint32_t)__shfl((int)r, __ffsll((long long)have) - 1, 64);
        const unsigned long long same = __ballot(r == lead);
        if (r == lead) { if (lane == __ffsll((long long)same) - 1) atomicAdd(&Cn[lead], (uint32_t)__popcll(same)); }
        else if (r != kVzNoLabel) atomicAdd(&Cn[r], 1u);
    }
}

__global__ __launch_bounds__(256) void vz_zone_emit_kernel(const VolzoneArgs A)
{
    __shared__ uint32_t s_T[(kVzLevelCap + 1) * kVzDenseSizes];
    const int tid = threadIdx.x;
    const VzRoi R = vz_roi(A, blockIdx.y);
    const VzRange g = vz_range(A, R);
    if (!g.any) return;
    const uint32_t rows = A.rows[VZ_GLSZM];
    for (uint32_t i = tid; i < rows * kVzDenseSizes; i += 256u) s_T[i] = 0u;
    __syncthreads();
    const unsigned char* const D = A.box[VZ_GLSZM] + (uint64_t)blockIdx.y * A.box_stride;
    const uint32_t* const Lb = A.sz_label + (uint64_t)blockIdx.y * A.cell_stride;
    const uint32_t* const Cn = A.sz_count + (uint64_t)blockIdx.y * A.cell_stride;
    uint32_t* const T = A.sz_tab + (uint64_t)blockIdx.y * A.sz_stride;
    uint32_t* const K = A.sz_keys + 2ull * blockIdx.y * A.key_stride;
    for (uint32_t i = g.c0 + (uint32_t)tid; i < g.c1; i += 256u) {
        if (Lb[i] != i) continue;                          // a root: the raster-first cell of its zone
        const uint32_t c = D[i], size = Cn[i];
        if (c >= rows || size == 0u || size > g.cells) { vz_internal(A); continue; }
        if (size <= kVzDenseSizes) atomicAdd(&s_T[c * kVzDenseSizes + (size - 1u)], 1u);
        else {
            const uint32_t pos = atomicAdd(&T[0], 1u);
            if ((uint64_t)pos < A.key_stride) K[pos] = ((size - 1u) << 8) | c;
            else vz_internal(A);                           // (more zones above kVzDenseSizes cells than cells / (kVzDenseSizes + 1))
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < rows * kVzDenseSizes; i += 256u) {
        const uint32_t v = s_T[i];
        if (v) atomicAdd(&T[kVzSzHead + i], v);
    }
}

// stable LSD radix sort of the ROI's list, four bits a pass over the bits the largest key has (the form of vol_intensity_kernel: thread
// t owns the keys [c0, c1) of every pass).  T[1] says which buffer holds the result.
__global__ __launch_bounds__(256) void vz_zone_sort_kernel(const VolzoneArgs A)
{
    __shared__ uint32_t s_cnt[16 * 256];
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_hi;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const VzRoi R = vz_roi(A, blockIdx.x);
    if (!vz_swept(A, R)) return;
    uint32_t* const T = A.sz_tab + (uint64_t)blockIdx.x * A.sz_stride;
    uint32_t n = T[0];
    if ((uint64_t)n > A.key_stride) n = (uint32_t)A.key_stride;          // (the emit kernel raised the status)
    if (n == 0u) return;
    uint32_t* src = A.sz_keys + 2ull * blockIdx.x * A.key_stride;
    uint32_t* dst = src + A.key_stride;
    if (tid == 0) s_hi = 0u;
    __syncthreads();
    uint32_t hi = 0;
    for (uint32_t i = tid; i < n; i += 256u) hi = src[i] > hi ? src[i] : hi;
    atomicMax(&s_hi, hi);
    __syncthreads();
    const int bits = 32 - __clz((int)(s_hi | 1u));
    const uint32_t cs = (n + 255u) / 256u;
    const uint32_t c0 = (uint64_t)tid * cs < n ? (uint32_t)tid * cs : n, c1 = (uint64_t)c0 + cs < n ? c0 + cs : n;
    uint32_t flips = 0;
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
        __threadfence_block();
        __syncthreads();
        uint32_t* const t = src; src = dst; dst = t;
        flips ^= 1u;
    }
    if (tid == 0) T[1] = flips;
}

// first index in [lo, n) whose key >> sh exceeds v >> sh (the list is sorted): at most 32 halvings
__device__ __forceinline__ uint32_t vz_upper(const uint32_t* K, uint32_t lo, uint32_t n, uint32_t v, int sh)
{
    uint32_t hi = n;
    for (int it = 0; it < 33 && lo < hi; it++) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((K[mid] >> sh) <= (v >> sh)) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// 3d_glszm.cpp:531-588, calc_sums_of_P and the calc_* functions.  Empty cells of the matrix add exactly 0 to every sum of this class, so
// the loops run over the cells that hold zones: the dense table in (level, size) order by flat index, then the sorted list.
__global__ __launch_bounds__(64) void vz_zone_close_kernel(const VolzoneArgs A)
{
    __shared__ uint32_t s_row[kVzLevelCap + 1];
    __shared__ double s_p[kVzSums][64];
    __shared__ double s_r[kVzSums];
    const int lane = threadIdx.x;
    const uint32_t rows = A.rows[VZ_GLSZM];
    const VzRoi R = vz_roi(A, blockIdx.x);
    double* const o = A.out + R.roi * A.ld + A.col[VZ_GLSZM];
    if (R.n64 == 0 || (R.vmin == R.vmax && R.cells != 0)) {            // no voxels; a flat ROI (3d_glszm.cpp:476-480)
        if (lane < kVzGlszmCols) o[lane] = A.soft_nan;
        return;
    }
    if (!vz_swept(A, R)) return;
    const uint32_t* const T = A.sz_tab + (uint64_t)blockIdx.x * A.sz_stride;
    const uint32_t* const Dn = T + kVzSzHead;
    uint32_t n = T[0];
    if ((uint64_t)n > A.key_stride) n = (uint32_t)A.key_stride;
    const uint32_t* const K = A.sz_keys + 2ull * blockIdx.x * A.key_stride + (T[1] ? A.key_stride : 0ull);
    for (uint32_t i = lane; i < rows; i += 64u) s_row[i] = 0u;
    __syncthreads();
    const uint32_t nd = rows * kVzDenseSizes;
    // pass 1: Nz, the row sums si, the sum of the squared column sums sj
    unsigned long long tot = 0, sq = 0;
    if ((uint32_t)lane < kVzDenseSizes) {
        uint32_t cs = 0;
        for (uint32_t i = 0; i < rows; i++) cs += Dn[i * kVzDenseSizes + lane];
        sq += (unsigned long long)cs * cs;
    }
    for (uint32_t e = lane; e < nd; e += 64u) {
        const uint32_t p = Dn[e];
        if (p) { tot += p; atomicAdd(&s_row[e / kVzDenseSizes], p); }
    }
    for (uint32_t e = lane; e < n; e += 64u) {
        const uint32_t key = K[e];
        if ((key & 255u) >= rows) { vz_internal(A); continue; }
        tot += 1ull;
        atomicAdd(&s_row[key & 255u], 1u);
        if (e == 0u || (K[e - 1u] >> 8) != (key >> 8)) {   // the first zone of its size
            const unsigned long long cs = vz_upper(K, e, n, key, 8) - e;
            sq += cs * cs;
        }
    }
    tot = vz_wave_sum_u64(tot);
    sq = vz_wave_sum_u64(sq);
    __syncthreads();
    if (tot == 0ull) {                                     // sum_p == 0: invalidate (3d_glszm.cpp:562-566)
        if (lane < kVzGlszmCols) o[lane] = A.soft_nan;
        return;
    }
    const double sum = (double)tot;
    // pass 2
    enum { SAE, LAE, MUZ, MUG, ZE, LAH, LAL, SAH, SAL, N2 };
    double a2[N2] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    auto term2 = [&](double p, double inten, double jj) {
        const double i2 = inten * inten, j2 = jj * jj;
        a2[SAE] += p / j2;
        a2[LAE] += p * j2;
        a2[LAH] += p * i2 * j2;
        a2[LAL] += p * j2 / i2;
        a2[SAH] += p * i2 / j2;
        a2[SAL] += p / (i2 * j2);
        a2[ZE] += p / sum * (fast_log10(p / sum + 2.2e-16) / 0.30102999566);
        a2[MUZ] += p / sum * jj;
        a2[MUG] += p / sum * inten;
    };
    for (uint32_t e = lane; e < nd; e += 64u) {
        const uint32_t p = Dn[e];
        if (p) term2((double)(int)p, (double)(e / kVzDenseSizes), (double)(e % kVzDenseSizes + 1u));
    }
    for (uint32_t e = lane; e < n; e += 64u) {
        const uint32_t key = K[e];
        if (e != 0u && K[e - 1u] == key) continue;         // the first zone of its (level, size) cell
        term2((double)(vz_upper(K, e, n, key, 0) - e), (double)(key & 255u), (double)((key >> 8) + 1u));
    }
    vz_lane_sums(a2, s_p, s_r, lane);
    const double sae = a2[SAE], lae = a2[LAE], muZ = a2[MUZ], muG = a2[MUG], ze = a2[ZE], lah = a2[LAH], lal = a2[LAL], sah = a2[SAH], sal = a2[SAL];
    // pass 3
    double a3[2] = {0.0, 0.0};
    auto term3 = [&](double p, double inten, double jj) {
        a3[0] += p / sum * ((inten - muG) * (inten - muG));
        a3[1] += p / sum * ((jj - muZ) * (jj - muZ));
    };
    for (uint32_t e = lane; e < nd; e += 64u) {
        const uint32_t p = Dn[e];
        if (p) term3((double)(int)p, (double)(e / kVzDenseSizes), (double)(e % kVzDenseSizes + 1u));
    }
    for (uint32_t e = lane; e < n; e += 64u) {
        const uint32_t key = K[e];
        if (e != 0u && K[e - 1u] == key) continue;
        term3((double)(vz_upper(K, e, n, key, 0) - e), (double)(key & 255u), (double)((key >> 8) + 1u));
    }
    vz_lane_sums(a3, s_p, s_r, lane);
    const double glv = a3[0], zv = a3[1];
    if (lane != 0) return;
    double gln = 0.0, lgl = 0.0, hgl = 0.0;
#pragma unroll 1
    for (uint32_t i = 1; i < rows; i++) {
        const double s = (double)s_row[i], inten = (double)i;
        gln += s * s;
        lgl += s / (inten * inten);
        hgl += s * (inten * inten);
    }
    const double szn = (double)sq;
    o[0] = sae / sum;                                      // (Nz: the same number)
    o[1] = lae / sum;
    o[2] = gln / sum;
    o[3] = gln / (sum * sum);
    o[4] = szn / sum;
    o[5] = szn / (sum * sum);
    o[6] = sum / (double)R.n64;
    o[7] = glv;
    o[8] = zv;
    o[9] = -ze;
    o[10] = lgl / sum;
    o[11] = hgl / sum;
    o[12] = sal / sum;
    o[13] = sah / sum;
    o[14] = lal / sum;
    o[15] = lah / sum;
}

dim3 vz_range_grid(const VolzoneArgs& a, uint32_t z) { return dim3((a.max_cells + kVzCellsPerWg - 1u) / kVzCellsPerWg, (uint32_t)a.n_roi, z); }

} // namespace

int launch_volzone_runs(const VolzoneArgs& a, void* stream)
{
    if (a.n_roi == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(vz_runs_kernel, vz_range_grid(a, kVzDirs), dim3(256), 0, st, a);
    if (int rc = (int)hipGetLastError()) return rc;
    hipLaunchKernelGGL(vz_runs_close_kernel, dim3(kVzDirs, (uint32_t)a.n_roi), dim3(64), 0, st, a);
    if (int rc = (int)hipGetLastError()) return rc;
    hipLaunchKernelGGL(vz_runs_ave_kernel, dim3((uint32_t)((a.n_roi * kVzGlrlmCodes + 255u) / 256u)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int launch_volzone_zone_step(const VolzoneArgs& a, int step, void* stream)
{
    if (a.n_roi == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    switch (step) {
    case 0: hipLaunchKernelGGL(vz_zone_init_kernel, vz_range_grid(a, 1), dim3(256), 0, st, a); break;
    case 1: hipLaunchKernelGGL(vz_zone_merge_kernel, vz_range_grid(a, 1), dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(vz_zone_count_kernel, vz_range_grid(a, 1), dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(vz_zone_emit_kernel, vz_range_grid(a, 1), dim3(256), 0, st, a); break;
    case 4: hipLaunchKernelGGL(vz_zone_sort_kernel, dim3((uint32_t)a.n_roi), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(vz_zone_close_kernel, dim3((uint32_t)a.n_roi), dim3(64), 0, st, a); break;
    }
    return (int)hipGetLastError();
}

int launch_volzone_zones(const VolzoneArgs& a, void* stream)
{
    for (int step = 0; step < kVzZoneSteps; step++)
        if (int rc = launch_volzone_zone_step(a, step, stream)) return rc;
    return 0;
}

} // namespace nyxhip
