// roi_voldzone.hip -- volumes (3-D): the GLDZM block of the reference's Feature3D enum (3d_gldzm.cpp), gfx950.
//
// The class reads a binned box of vol_bin_kernel (roi_vol.hip).  THE RULING: a cell of level 0 forms no zone and is
// always a border, in every binning mode, as the reference treats it in IBSI mode; everything else is the text of 3d_gldzm.cpp.
//
//   vdz_dist_y_kernel   a thread per (z, x) column of the box (lanes across x): it walks y forward and backward and carries the nearest
//                       border -- a level-0 cell or the box face -- so a cell costs two steps whatever the box side.  Stores
//                       min(up, down) of dist2border (3d_gldzm.cpp:330-375) in 16 bits (roi_voldzone.h: the bound of the metric).
//   vdz_dist_x_kernel   a wave per group of whole rows: 64 cells a trip in raster order; the nearest border to the left of a lane is the
//                       highest set bit below it in the ballots of (x == 0, own lane included) and (level 0, own lane excluded), else
//                       the carry of the trips before; to the right likewise in a second sweep from the far end.  The map is static: the
//                       reference's VISITED marks are non-zero and never borders.
//   vdz_init_kernel     label = own cell index; level-0 cells get kVzNoLabel; the minimum per cell starts at the largest word
//   vdz_merge_kernel    each cell unites with its 3 raster-earlier face neighbours (-x, -y, -z) of equal level: a zone is a 6-connected
//                       component (the reference's walk goes E, S, W, N, +z, -z); the union-find chain of vol_zone_prims.h
//   vdz_min_kernel      each cell chases its root (and stores it), then atomicMins its distance into the root (a wave joins its lanes
//                       of the leading root in one atomic): the zone metric
//   vdz_emit_kernel     each root counts [level][metric - 1] in the ROI's table (pitch vdz_pitch(w, h)): metrics up to kVdzShortDist in
//                       LDS, merged with integer atomics, larger ones in the global table directly; the largest metric is Nd
//   vdz_close_kernel    a wave per ROI: lanes own the distances lane + 1, lane + 65, ..; row sums Mx, column sums Md and Ns are
//                       integers; per-lane fp64 partials are added in lane order by one lane (calc_features, 3d_gldzm.cpp:407-502)
//
// An ROI has ceil(cells / kVzCellsPerWg) workgroups per cell sweep, each owning a fixed range of cells of the ROI's own box; surplus
// workgroups leave at once.  No kernel waits for another workgroup: the order between the phases is the order of the launches on the
// stream.  Every loop is bounded by the box; a chase that reaches its bound raises NYXHIP_ERR_INTERNAL.  Everything more than one thread
// adds to is an integer.  Nothing of an ROI's row depends on another ROI.  Built with -ffp-contract=off (device_math.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "device_math.h"
#include "launch_util.h"
#include "roi_vol.h"
#include "roi_voldzone.h"
#include "vol_zone_prims.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

struct VdRoi {
    uint64_t roi, n64;
    uint32_t w, h, d, vmin, vmax;
    uint64_t cells;
};
__device__ __forceinline__ VdRoi vd_roi(const VoldzoneArgs& A, uint32_t j)
{
    VdRoi R;
    R.roi = A.roi0 + j;
    R.n64 = A.px_offset[R.roi + 1] - A.px_offset[R.roi];
    R.w = A.bbox_w[R.roi]; R.h = A.bbox_h[R.roi]; R.d = A.bbox_d[R.roi];
    R.vmin = A.vmin[R.roi]; R.vmax = A.vmax[R.roi];
    const bool sides = R.w <= kVolMaxSide && R.h <= kVolMaxSide && R.d <= kVolMaxSide;
    R.cells = sides ? (uint64_t)R.w * R.h * R.d : ~0ull;
    return R;
}
// what the sweeps touch: an ROI with voxels that is not flat, inside what the strides were sized for (vol_bin_kernel raises the status
// of the others)
__device__ __forceinline__ bool vd_swept(const VoldzoneArgs& A, const VdRoi& R)
{
    return R.n64 != 0 && R.cells != 0 && R.cells <= (uint64_t)A.max_cells && R.cells <= (uint64_t)kVolMaxCells && R.vmin != R.vmax &&
           R.w <= A.side_max[0] && R.h <= A.side_max[1] && R.d <= A.side_max[2] && vdz_pitch(R.w, R.h) <= A.pitch_max;
}
__device__ __forceinline__ bool vd_blank(const VdRoi& R) { return R.n64 == 0 || (R.vmin == R.vmax && R.cells != 0); }

// ---- the distance map -------------------------------------------------------------------------------------------------------------
// dist2border, the y half: per direction the distance to the nearest cell that is level 0 or lies on the box face, a cell on the face
// itself 0; then + 1 (3d_gldzm.cpp:348-368).  With `last` = the nearest such position before y (0 when there is none) that is
// y - last + 1 for every y, the face cell included.
__global__ __launch_bounds__(256) void vdz_dist_y_kernel(const VoldzoneArgs A)
{
    const VdRoi R = vd_roi(A, blockIdx.y);
    if (!vd_swept(A, R)) return;
    const uint32_t cols = R.w * R.d, wh = R.w * R.h;
    const unsigned char* const D = A.box + (uint64_t)blockIdx.y * A.box_stride;
    uint16_t* const Dm = A.dist + (uint64_t)blockIdx.y * A.dist_stride;
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < (uint64_t)cols; t += (uint64_t)gridDim.x * 256u) {
        const uint32_t z = (uint32_t)t / R.w, x = (uint32_t)t - z * R.w, base = z * wh + x;
        uint32_t last = 0;
        for (uint32_t y = 0; y < R.h; y++) {
            const uint32_t i = base + y * R.w;
            Dm[i] = (uint16_t)(y - last + 1u);
            if (D[i] == 0) last = y;
        }
        uint32_t next = R.h - 1u;
        for (uint32_t y = R.h; y-- > 0u;) {
            const uint32_t i = base + y * R.w, db = next - y + 1u;
            if (db < (uint32_t)Dm[i]) Dm[i] = (uint16_t)db;
            if (D[i] == 0) next = y;
        }
    }
}

// the x half (3d_gldzm.cpp:332-347), over the cells of whole rows in raster order: the row start x == 0 is the border of its own cell
// and of every cell to its right, so a border of an earlier row never reaches into the next one
__global__ __launch_bounds__(256) void vdz_dist_x_kernel(const VoldzoneArgs A)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const VdRoi R = vd_roi(A, blockIdx.y);
    if (!vd_swept(A, R)) return;
    const unsigned char* const D = A.box + (uint64_t)blockIdx.y * A.box_stride;
    uint16_t* const Dm = A.dist + (uint64_t)blockIdx.y * A.dist_stride;
    const uint32_t nrows = R.h * R.d, rpw = vdz_rows_per_wave(R.w), jobs = (nrows + rpw - 1u) / rpw;
    const unsigned long long own = 1ull << lane, below = own - 1ull, above = ~(below | own);
    for (uint64_t job = (uint64_t)blockIdx.x * 4u + (uint32_t)wave; job < (uint64_t)jobs; job += (uint64_t)gridDim.x * 4u) {
        const uint32_t r0 = (uint32_t)job * rpw, r1 = nrows - r0 > rpw ? r0 + rpw : nrows;
        const uint32_t c0 = r0 * R.w, c1 = r1 * R.w, trips = (c1 - c0 + 63u) / 64u;
        uint32_t carry = c0;                               // the nearest border at or before the trip: the first row's start
        for (uint32_t k = 0; k < trips; k++) {
            const uint32_t b = c0 + k * 64u, i = b + (uint32_t)lane;
            const bool valid = i < c1;
            const uint32_t x = valid ? i % R.w : 1u;
            const bool zero = valid && D[i] == 0;
            const unsigned long long face = __ballot(valid && x == 0u), hole = __ballot(zero);
            const unsigned long long m = (face & (below | own)) | (hole & below);
            const uint32_t last = m ? b + 63u - (uint32_t)__clzll((long long)m) : carry;
            if (valid) {
                const uint32_t dl = i - last + 1u;
                if (dl < (uint32_t)Dm[i]) Dm[i] = (uint16_t)dl;
            }
            const unsigned long long all = face | hole;
            if (all) carry = b + 63u - (uint32_t)__clzll((long long)all);
        }
        carry = c1 - 1u;                                   // the nearest border at or after the trip: the last row's end
        for (uint32_t k = trips; k-- > 0u;) {
            const uint32_t b = c0 + k * 64u, i = b + (uint32_t)lane;
            const bool valid = i < c1;
            const uint32_t x = valid ? i % R.w : 0u;
            const bool zero = valid && D[i] == 0;
            const unsigned long long face = __ballot(valid && x == R.w - 1u), hole = __ballot(zero);
            const unsigned long long m = (face & (above | own)) | (hole & above);
            const uint32_t next = m ? b + (uint32_t)__ffsll((long long)m) - 1u : carry;
            if (valid) {
                const uint32_t dr = next - i + 1u;
                if (dr < (uint32_t)Dm[i]) Dm[i] = (uint16_t)dr;
            }
            const unsigned long long all = face | hole;
            if (all) carry = b + (uint32_t)__ffsll((long long)all) - 1u;
        }
    }
}

// ---- zones ------------------------------------------------------------------------------------------------------------------------
struct VdRange { uint32_t cells, c0, c1; bool any; };
__device__ __forceinline__ VdRange vd_range(const VoldzoneArgs& A, const VdRoi& R)
{
    VdRange g{0u, 0u, 0u, false};
    if (!vd_swept(A, R)) return g;
    g.cells = (uint32_t)R.cells;
    if ((uint64_t)blockIdx.x * kVzCellsPerWg >= (uint64_t)g.cells) return g;
    g.c0 = blockIdx.x * kVzCellsPerWg;
    g.c1 = g.cells - g.c0 > kVzCellsPerWg ? g.c0 + kVzCellsPerWg : g.cells;
    g.any = true;
    return g;
}

__global__ __launch_bounds__(256) void vdz_init_kernel(const VoldzoneArgs A)
{
    const VdRoi R = vd_roi(A, blockIdx.y);
    const VdRange g = vd_range(A, R);
    if (!g.any) return;
    const unsigned char* const D = A.box + (uint64_t)blockIdx.y * A.box_stride;
    uint32_t* const Lb = A.label + (uint64_t)blockIdx.y * A.cell_stride;
    uint32_t* const Zm = A.zmin + (uint64_t)blockIdx.y * A.cell_stride;
    for (uint32_t i = g.c0 + threadIdx.x; i < g.c1; i += 256u) {
        Lb[i] = D[i] == 0 ? kVzNoLabel : i;                // level 0 only: the background of matlab binning is level 1 and forms zones
        Zm[i] = 0xFFFFFFFFu;
    }
}

__global__ __launch_bounds__(256) void vdz_merge_kernel(const VoldzoneArgs A)
{
    const VdRoi R = vd_roi(A, blockIdx.y);
    const VdRange g = vd_range(A, R);
    if (!g.any) return;
    const unsigned char* const D = A.box + (uint64_t)blockIdx.y * A.box_stride;
    uint32_t* const Lb = A.label + (uint64_t)blockIdx.y * A.cell_stride;
    const uint32_t wh = R.w * R.h;
    for (uint32_t i = g.c0 + threadIdx.x; i < g.c1; i += 256u) {
        const uint32_t c = D[i];
        if (c == 0u) continue;
        const uint32_t z = i / wh, rem = i - z * wh, y = rem / R.w, x = rem - y * R.w;
        // two cells that already point at the same parent are united: inside a large zone (the background of matlab binning is one)
        // most pairs are, and the check spares both chases their reads of the one root every cell of the zone ends at
        if (x > 0u && D[i - 1u] == c && vz_ld(&Lb[i]) != vz_ld(&Lb[i - 1u])) vz_unite(A.status, Lb, i, i - 1u, g.cells);
        if (y > 0u && D[i - R.w] == c && vz_ld(&Lb[i]) != vz_ld(&Lb[i - R.w])) vz_unite(A.status, Lb, i, i - R.w, g.cells);
        if (z > 0u && D[i - wh] == c && vz_ld(&Lb[i]) != vz_ld(&Lb[i - wh])) vz_unite(A.status, Lb, i, i - wh, g.cells);
    }
}

__global__ __launch_bounds__(256) void vdz_min_kernel(const VoldzoneArgs A)
{
    const VdRoi R = vd_roi(A, blockIdx.y);
    const VdRange g = vd_range(A, R);
    if (!g.any) return;
    uint32_t* const Lb = A.label + (uint64_t)blockIdx.y * A.cell_stride;
    uint32_t* const Zm = A.zmin + (uint64_t)blockIdx.y * A.cell_stride;
    const uint16_t* const Dm = A.dist + (uint64_t)blockIdx.y * A.dist_stride;
    const int lane = threadIdx.x & 63;
    for (uint32_t i0 = g.c0; i0 < g.c1; i0 += 256u) {      // (the trip count is the workgroup's: every lane reaches the ballots)
        const uint32_t i = i0 + threadIdx.x;
        uint32_t r = kVzNoLabel, dv = 0xFFFFFFFFu;
        if (i < g.c1 && vz_ld(&Lb[i]) != kVzNoLabel) {
            uint32_t budget = g.cells;
            r = vz_find(A.status, Lb, i, g.cells, budget);
            __hip_atomic_store(&Lb[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a root keeps its own index)
            dv = Dm[i];
        }
        const unsigned long long have = __ballot(r != kVzNoLabel);
        if (have == 0ull) continue;
        const uint32_t lead = (uint32_t)__shfl((int)r, __ffsll((long long)have) - 1, 64);
        const unsigned long long same = __ballot(r == lead);
        uint32_t mn = r == lead ? dv : 0xFFFFFFFFu;
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)mn, o, 64);
            mn = other < mn ? other : mn;
        }
        // a minimum only falls, so a value that is not below the one read cannot change it: the cells of a large zone then cost its
        // root a read, not an atomic apiece
        if (r == lead) { if (lane == __ffsll((long long)same) - 1 && mn < vz_ld(&Zm[lead])) atomicMin(&Zm[lead], mn); }
        else if (r != kVzNoLabel && dv < vz_ld(&Zm[r])) atomicMin(&Zm[r], dv);
    }
}

__global__ __launch_bounds__(256) void vdz_emit_kernel(const VoldzoneArgs A)
{
    __shared__ uint32_t s_T[(kVzLevelCap + 1) * kVdzShortDist];
    __shared__ uint32_t s_max;
    const int tid = threadIdx.x;
    const VdRoi R = vd_roi(A, blockIdx.y);
    const VdRange g = vd_range(A, R);
    if (!g.any) return;
    const uint32_t rows = A.rows, P = vdz_pitch(R.w, R.h);
    for (uint32_t i = tid; i < rows * kVdzShortDist; i += 256u) s_T[i] = 0u;
    if (tid == 0) s_max = 0u;
    __syncthreads();
    const unsigned char* const D = A.box + (uint64_t)blockIdx.y * A.box_stride;
    const uint32_t* const Lb = A.label + (uint64_t)blockIdx.y * A.cell_stride;
    const uint32_t* const Zm = A.zmin + (uint64_t)blockIdx.y * A.cell_stride;
    uint32_t* const T = A.tab + (uint64_t)blockIdx.y * A.tab_stride;
    uint32_t* const G = T + kVdzHead;
    uint32_t largest = 0;
    for (uint32_t i = g.c0 + (uint32_t)tid; i < g.c1; i += 256u) {
        if (Lb[i] != i) continue;                          // a root: the raster-first cell of its zone
        const uint32_t c = D[i], m = Zm[i];
        if (c == 0u || c >= rows || m == 0u || m > P) { vz_raise_internal(A.status); continue; }
        if (m <= kVdzShortDist) atomicAdd(&s_T[c * kVdzShortDist + (m - 1u)], 1u);
        else atomicAdd(&G[(uint64_t)c * P + (m - 1u)], 1u);
        largest = m > largest ? m : largest;
    }
    if (largest) atomicMax(&s_max, largest);
    __syncthreads();
    for (uint32_t i = tid; i < rows * kVdzShortDist; i += 256u) {
        const uint32_t v = s_T[i];
        if (v == 0u) continue;
        const uint32_t c = i / kVdzShortDist, j = i - c * kVdzShortDist;   // (j < P: a zone of that metric was met)
        atomicAdd(&G[(uint64_t)c * P + j], v);
    }
    if (tid == 0 && s_max) atomicMax(&T[0], s_max);
}

// calc_row_and_column_sum_vectors and calc_features (3d_gldzm.cpp:377-502).  The matrix is [level][metric - 1]; row 0 holds nothing (the
// ruling), rows of absent levels and columns beyond Nd are empty and add exactly 0 to every sum (the entropy term too: 0 * log2(EPS)),
// so the loops run over the table rows and skip empty cells.
__global__ __launch_bounds__(64) void vdz_close_kernel(const VoldzoneArgs A)
{
    __shared__ uint32_t s_row[kVzLevelCap + 1];
    __shared__ double s_p[kVzSums][64];
    __shared__ double s_r[kVzSums];
    const int lane = threadIdx.x;
    const uint32_t rows = A.rows;
    const VdRoi R = vd_roi(A, blockIdx.x);
    double* const o = A.out + R.roi * A.ld;
    if (vd_blank(R)) {                                     // no voxels; a flat ROI (3d_gldzm.cpp:509-533)
        if (lane < kVdzCols) o[lane] = A.soft_nan;
        return;
    }
    if (!vd_swept(A, R)) return;                           // (the binning kernel raised the status)
    const uint32_t P = vdz_pitch(R.w, R.h);
    const uint32_t* const T = A.tab + (uint64_t)blockIdx.x * A.tab_stride;
    const uint32_t* const G = T + kVdzHead;
    uint32_t Nd = T[0];
    if (Nd > P) { if (lane == 0) vz_raise_internal(A.status); Nd = P; }
    for (uint32_t i = lane; i < rows; i += 64u) s_row[i] = 0u;
    __syncthreads();
    // pass 1: the row sums Mx and Ns, integers
    unsigned long long tot = 0;
    for (uint32_t j = lane; j < Nd; j += 64u)
        for (uint32_t i = 1; i < rows; i++) {
            const uint32_t p = G[(uint64_t)i * P + j];
            if (p) { tot += p; atomicAdd(&s_row[i], p); }
        }
    tot = vz_wave_sum_u64(tot);
    const double Ns = (double)tot;
    // pass 2: the sums over the distances (of Md) and over the cells
    enum { SDE, LDE, ZDNU, SDL, SDH, LDL, LDH, GLM, ZDM, ZDE, N2 };
    double a2[N2] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t j = lane; j < Nd; j += 64u) {
        const double dd = (double)(j + 1u);
        uint32_t cs = 0;
        for (uint32_t i = 1; i < rows; i++) {
            const uint32_t pi = G[(uint64_t)i * P + j];
            if (pi == 0u) continue;
            cs += pi;
            const double p = (double)pi, gg = (double)i;
            a2[SDL] += p / gg / gg / dd / dd;
            a2[SDH] += gg * gg * p / dd / dd;
            a2[LDL] += dd * dd * p / gg / gg;
            a2[LDH] += gg * gg * dd * dd * p;
            a2[GLM] += gg * p;
            a2[ZDM] += dd * p;
            a2[ZDE] += p / Ns * log2(p / Ns + 2.2e-16);
        }
        const double m = (double)cs;
        a2[SDE] += m / dd / dd;
        a2[LDE] += dd * dd * m;
        a2[ZDNU] += m * m;
    }
    vz_lane_sums(a2, s_p, s_r, lane);
    const double glm = a2[GLM] / Ns, zdm = a2[ZDM] / Ns;
    // pass 3: the variances about the two means
    double a3[2] = {0.0, 0.0};
    for (uint32_t j = lane; j < Nd; j += 64u) {
        const double dd = (double)(j + 1u);
        for (uint32_t i = 1; i < rows; i++) {
            const uint32_t pi = G[(uint64_t)i * P + j];
            if (pi == 0u) continue;
            const double p = (double)pi / Ns, dg = (double)i - glm, dz = dd - zdm;
            a3[0] += dg * dg * p;
            a3[1] += dz * dz * p;
        }
    }
    vz_lane_sums(a3, s_p, s_r, lane);
    if (lane != 0) return;
    double lgl = 0.0, hgl = 0.0, glnu = 0.0;
#pragma unroll 1
    for (uint32_t i = 1; i < rows; i++) {
        const double x = (double)s_row[i], gg = (double)i;
        if (x == 0.0) continue;
        lgl += x / (gg * gg);
        hgl += (gg * gg) * x;
        glnu += x * x;
    }
    const double zdnu = a2[ZDNU] / Ns;
    glnu /= Ns;
    o[0] = a2[SDE] / Ns;
    o[1] = a2[LDE] / Ns;
    o[2] = lgl / Ns;
    o[3] = hgl / Ns;
    o[4] = a2[SDL] / Ns;
    o[5] = a2[SDH] / Ns;
    o[6] = a2[LDL] / Ns;
    o[7] = a2[LDH] / Ns;
    o[8] = glnu;
    o[9] = glnu / Ns;
    o[10] = zdnu;
    o[11] = zdnu / Ns;
    o[12] = Ns / (double)(unsigned int)R.n64;              // ZP = Ns / aux_area
    o[13] = glm;
    o[14] = a3[0];
    o[15] = zdm;
    o[16] = a3[1];
    o[17] = -a2[ZDE];
}

uint32_t cap_grid(uint64_t n) { return (uint32_t)(n < 1u ? 1u : n > 65536u ? 65536u : n); }
dim3 vd_range_grid(const VoldzoneArgs& a) { return dim3((a.max_cells + kVzCellsPerWg - 1u) / kVzCellsPerWg, (uint32_t)a.n_roi, 1); }

} // namespace

int launch_voldzone_step(const VoldzoneArgs& a, int step, void* stream)
{
    if (a.n_roi == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nr = (uint32_t)a.n_roi;
    switch (step) {
    case 0: {
        const uint64_t cols = std::min<uint64_t>(a.max_cells, (uint64_t)a.side_max[0] * a.side_max[2]);
        hipLaunchKernelGGL(vdz_dist_y_kernel, dim3(cap_grid((cols + 255u) / 256u), nr), dim3(256), 0, st, a);
        break;
    }
    case 1: {
        const uint64_t jobs = (uint64_t)a.max_cells / (kVdzRowCells / 2u) + 1u;   // a job holds more than kVdzRowCells / 2 cells, but for the last
        hipLaunchKernelGGL(vdz_dist_x_kernel, dim3(cap_grid((jobs + 3u) / 4u), nr), dim3(256), 0, st, a);
        break;
    }
    case 2: hipLaunchKernelGGL(vdz_init_kernel, vd_range_grid(a), dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(vdz_merge_kernel, vd_range_grid(a), dim3(256), 0, st, a); break;
    case 4: hipLaunchKernelGGL(vdz_min_kernel, vd_range_grid(a), dim3(256), 0, st, a); break;
    case 5: hipLaunchKernelGGL(vdz_emit_kernel, vd_range_grid(a), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(vdz_close_kernel, dim3(nr), dim3(64), 0, st, a); break;
    }
    return (int)hipGetLastError();
}

int launch_voldzone(const VoldzoneArgs& a, void* stream)
{
    for (int step = 0; step < kVdzSteps; step++)
        if (int rc = launch_voldzone_step(a, step, stream)) return rc;
    return 0;
}

} // namespace nyxhip
