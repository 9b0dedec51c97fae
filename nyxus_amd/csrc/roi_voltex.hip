// roi_voltex.hip -- volumes (3-D): the GLDM, NGLDM and NGTDM blocks of the reference's Feature3D enum (gfx950).
//
//   voltex_bin_ngldm_kernel  NGLDM's own binned box: to_grayscale(v, 0, aux_max, grey_depth, ibsi) per voxel (3d_ngldm.cpp:88-101, :137);
//                            a cell outside the cloud holds to_grayscale(0) = 0 (the caller fills the boxes with it).  GLDM and NGTDM
//                            take their boxes from vol_bin_kernel (roi_vol.hip).
//   voltex_sweep_kernel<C>   an ROI has ceil(cells / kVtCellsPerWg) workgroups, each owning a fixed range of cells of the ROI's own box.
//                            A workgroup accumulates its part of the ROI's table (roi_voltex.h) in LDS with integer atomics and merges
//                            what is not zero into the per-ROI global table with integer atomics:
//                              GLDM   (3d_gldm.cpp:120-150)   a cell that is not the background level counts itself and the equal ones of
//                                     26 shifts: table[level][nd - 1]++
//                              NGLDM  (3d_ngldm.cpp:123-162)  every interior cell of the box, off-ROI cells too, counts the equal ones of
//                                     24 shifts (none straight up or down): table[level][matches]++
//                              NGTDM  (3d_ngtdm.cpp:69-121)   every cell that is not the background level, over the cube of the radius
//                                     clipped to the box (nd cells besides itself, background cells summed too): count[level]++ and
//                                     sum[level][class] += |nd * i - sum of the neighbours|, class = how many cells the cube has inside
//                                     the box along each axis, so nd is the same for all entries of a class
//                            and the presence map of the levels of ALL cells of its range.
//   voltex_ngtdm_r0_kernel   NGTDM at radius 0: no cell has a neighbour, the table is empty; the level count comes from the cloud
//   voltex_close_kernel      a wave per (ROI, column): the table into LDS, then lane 0 runs the reference's loop of that column term by
//                            term in fp64 (3d_gldm.cpp:270-553, 3d_ngldm.cpp:259-360, 3d_ngtdm.cpp:422-536)
//
// Everything that more than one thread adds to is an integer; every floating-point sum runs in the reference's order on one lane.
// Nothing of an ROI's row depends on another ROI.  Built with -ffp-contract=off (device_math.h).
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "launch_util.h"
#include "roi_vol.h"
#include "roi_voltex.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

struct VtRoi {
    uint64_t roi, off, n64;
    uint32_t w, h, d, vmin, vmax;
    uint64_t cells;
};
__device__ __forceinline__ VtRoi vt_roi(const VoltexArgs& A, uint32_t j)
{
    VtRoi R;
    R.roi = A.roi0 + j;
    R.off = A.px_offset[R.roi];
    R.n64 = A.px_offset[R.roi + 1] - R.off;
    R.w = A.bbox_w[R.roi]; R.h = A.bbox_h[R.roi]; R.d = A.bbox_d[R.roi];
    R.vmin = A.vmin[R.roi]; R.vmax = A.vmax[R.roi];
    const bool sides = R.w <= kVolMaxSide && R.h <= kVolMaxSide && R.d <= kVolMaxSide;
    R.cells = sides ? (uint64_t)R.w * R.h * R.d : ~0ull;
    return R;
}
// what no kernel of the unit touches (the binning kernels raise the status): beyond what the strides were sized for
__device__ __forceinline__ bool vt_box_fits(const VoltexArgs& A, const VtRoi& R) { return R.cells <= (uint64_t)A.max_cells && R.cells <= (uint64_t)kVolMaxCells; }

__global__ __launch_bounds__(256) void voltex_bin_ngldm_kernel(const VoltexArgs A)
{
    const int tid = threadIdx.x;
    const VtRoi R = vt_roi(A, blockIdx.y);
    if (R.n64 == 0) return;
    const bool first = tid == 0 && blockIdx.x == 0;
    if (R.cells == 0) { if (first) atomicCAS(A.status, 0, NYXHIP_ERR_INVALID_ARG); return; }
    if (!vt_box_fits(A, R)) { if (first) atomicCAS(A.status, 0, NYXHIP_ERR_ROI_TOO_LARGE); return; }
    if (R.vmax == R.vmin) return;                          // a flat ROI is soft_nan before any level is read (3d_ngldm.cpp:173)
    if (A.ibsi && R.vmax > kVtLevelCap) { if (first) atomicCAS(A.status, 0, NYXHIP_ERR_UNSUPPORTED); return; }
    unsigned char* const box = A.box[VT_NGLDM] + (uint64_t)blockIdx.y * A.box_stride;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + (uint64_t)tid; i < R.n64; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t x = A.x[R.off + i], y = A.y[R.off + i], z = A.z[R.off + i];
        if (x >= R.w || y >= R.h || z >= R.d) { atomicCAS(A.status, 0, NYXHIP_ERR_INVALID_ARG); continue; }   // never stored
        const uint32_t v = A.inten[R.off + i];
        uint32_t lvl = A.ibsi ? v : to_grayscale(v, 0u, R.vmax, A.ngldm_levels);
        if (lvl > kVtLevelCap) { atomicCAS(A.status, 0, NYXHIP_ERR_UNSUPPORTED); lvl = 0; }                   // an intensity above the stated maximum
        box[((uint32_t)z * R.h + y) * R.w + x] = (unsigned char)lvl;
    }
}

template <int CLS> __host__ __device__ inline uint32_t vt_words(int radius)
{
    return CLS == VT_GLDM ? kVtGldmWords : CLS == VT_NGLDM ? kVtNgldmWords : vt_ngtdm_words(radius);
}

template <int CLS> __global__ __launch_bounds__(256) void voltex_sweep_kernel(const VoltexArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    uint32_t* const T = (uint32_t*)lds_raw;
    const int tid = threadIdx.x;
    const VtRoi R = vt_roi(A, blockIdx.y);
    if (R.n64 == 0 || R.cells == 0 || !vt_box_fits(A, R)) return;
    const uint32_t cells = (uint32_t)R.cells;
    if ((uint64_t)blockIdx.x * kVtCellsPerWg >= (uint64_t)cells) return;
    const uint32_t c0 = blockIdx.x * kVtCellsPerWg, c1 = cells - c0 > kVtCellsPerWg ? c0 + kVtCellsPerWg : cells;
    const int r = A.radius;
    const uint32_t ncls = vt_classes(r), words = vt_words<CLS>(r);
    for (uint32_t i = tid; i < words; i += 256u) T[i] = 0u;
    __syncthreads();
    const unsigned char* const D = A.box[CLS] + (uint64_t)blockIdx.y * A.box_stride;
    const int w = (int)R.w, h = (int)R.h, d = (int)R.d;
    const uint32_t wh = R.w * R.h;
    // the background level of the class's binning (3d_gldm.cpp:117, 3d_ngtdm.cpp:230): matlab binning maps 0 to 1.  NGTDM under the other
    // binnings skips nothing: either the box holds no 0, or the class has added 1 to every cell and 0 matches nothing (:221-227)
    const uint32_t zeroI = CLS == VT_GLDM ? (A.g_gldm > 0 ? 1u : 0u) : (A.g_ngtdm > 0 ? 1u : 0xFFFFFFFFu);
    unsigned long long* const S = (unsigned long long*)(T + kVtNgtdmSums);
    for (uint32_t i = c0 + (uint32_t)tid; i < c1; i += 256u) {
        const uint32_t uz = i / wh, rem = i - uz * wh, uy = rem / R.w;
        const int z = (int)uz, y = (int)uy, x = (int)(rem - uy * R.w);
        const uint32_t c = D[i];
        if (c > kVtLevelCap) continue;                     // (cannot hold: the binning kernels store no such level)
        atomicOr(&T[c >> 5], 1u << (c & 31u));
        if (CLS == VT_GLDM) {
            if (c == zeroI) continue;
            uint32_t nd = 0;
            for (int dz = -1; dz <= 1; dz++) {
                const int nz = z + dz;
                if (nz < 0 || nz >= d) continue;
                for (int dy = -1; dy <= 1; dy++) {
                    const int ny = y + dy;
                    if (ny < 0 || ny >= h) continue;
                    const unsigned char* const row = D + ((uint32_t)nz * R.h + (uint32_t)ny) * R.w;
                    for (int dx = -1; dx <= 1; dx++) {
                        const int nx = x + dx;
                        if (nx < 0 || nx >= w) continue;
                        nd += row[nx] == c ? 1u : 0u;       // (the voxel itself is one of the 27: nd starts at 1 in the reference)
                    }
                }
            }
            atomicAdd(&T[kVtTabHead + c * kVtGldmDeps + (nd - 1u)], 1u);
        } else if (CLS == VT_NGLDM) {
            if (x < 1 || x + 1 >= w || y < 1 || y + 1 >= h || z < 1 || z + 1 >= d) continue;   // border cells of the box (:123-127)
            uint32_t nm = 0;
            for (int dz = -1; dz <= 1; dz++)
                for (int dy = -1; dy <= 1; dy++) {
                    const unsigned char* const row = D + ((uint32_t)(z + dz) * R.h + (uint32_t)(y + dy)) * R.w;
                    for (int dx = -1; dx <= 1; dx++)
                        if (dx != 0 || dy != 0) nm += row[x + dx] == c ? 1u : 0u;              // (no straight up / down shift in shifts[])
                }
            atomicAdd(&T[kVtTabHead + c * kVtNgldmDeps + nm], 1u);
        } else {
            if (c == zeroI) continue;
            const int x0 = x - r < 0 ? 0 : x - r, x1 = x + r >= w ? w - 1 : x + r;
            const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r >= h ? h - 1 : y + r;
            const int z0 = z - r < 0 ? 0 : z - r, z1 = z + r >= d ? d - 1 : z + r;
            const int cx = x1 - x0 + 1, cy = y1 - y0 + 1, cz = z1 - z0 + 1;
            const int nd = cx * cy * cz - 1;
            if (nd <= 0) continue;                         // no neighbour: not a zone (:113)
            uint32_t sum = 0;
            for (int zz = z0; zz <= z1; zz++)
                for (int yy = y0; yy <= y1; yy++) {
                    const unsigned char* const row = D + ((uint32_t)zz * R.h + (uint32_t)yy) * R.w;
                    for (int xx = x0; xx <= x1; xx++) sum += row[xx];
                }
            sum -= c;
            // the class: cells of the cube inside the box along each axis, counted from the fewest a cell of this box can have
            int ax = cx - ((w - 1 < r ? w - 1 : r) + 1), ay = cy - ((h - 1 < r ? h - 1 : r) + 1), az = cz - ((d - 1 < r ? d - 1 : r) + 1);
            ax = ax < 0 ? 0 : ax > r ? r : ax; ay = ay < 0 ? 0 : ay > r ? r : ay; az = az < 0 ? 0 : az > r ? r : az;
            const uint32_t cls = ((uint32_t)az * (uint32_t)(r + 1) + (uint32_t)ay) * (uint32_t)(r + 1) + (uint32_t)ax;
            const long long df = (long long)nd * (long long)c - (long long)sum;
            atomicAdd(&T[kVtTabHead + c], 1u);
            atomicAdd(&S[c * ncls + cls], (unsigned long long)(df < 0 ? -df : df));
        }
    }
    __syncthreads();
    uint32_t* const G = A.tab[CLS] + (uint64_t)blockIdx.y * A.tab_stride[CLS];
    const uint32_t w32 = CLS == VT_NGTDM ? kVtNgtdmSums : words;
    for (uint32_t i = tid; i < w32; i += 256u) {
        const uint32_t v = T[i];
        if (v == 0u) continue;
        if (i < kVtTabHead) atomicOr(&G[i], v); else atomicAdd(&G[i], v);
    }
    if (CLS == VT_NGTDM) {
        unsigned long long* const GS = (unsigned long long*)(G + kVtNgtdmSums);
        for (uint32_t i = tid; i < kVtRows * ncls; i += 256u) {
            const unsigned long long v = S[i];
            if (v) atomicAdd(&GS[i], v);
        }
    }
}

__global__ __launch_bounds__(256) void voltex_ngtdm_r0_kernel(const VoltexArgs A)
{
    __shared__ uint32_t s_lo, s_hi;
    const int tid = threadIdx.x;
    const VtRoi R = vt_roi(A, blockIdx.x);
    double* const o = A.out + R.roi * A.ld + A.col_ngtdm;
    if (R.n64 == 0) { if (tid < kVtNgtdmCols) o[tid] = A.soft_nan; return; }
    if (R.cells == 0) { if (tid == 0) atomicCAS(A.status, 0, NYXHIP_ERR_INVALID_ARG); return; }
    if (!vt_box_fits(A, R)) { if (tid == 0) atomicCAS(A.status, 0, NYXHIP_ERR_ROI_TOO_LARGE); return; }
    if (tid == 0) { s_lo = 0xFFFFFFFFu; s_hi = 0u; }
    __syncthreads();
    const int g = A.g_ngtdm;
    const bool flat = g < 0 && R.vmax == R.vmin;           // (as vol_bin_kernel: every level is 0)
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (uint64_t i = tid; i < R.n64; i += 256u) {
        if (A.x[R.off + i] >= R.w || A.y[R.off + i] >= R.h || A.z[R.off + i] >= R.d) { atomicCAS(A.status, 0, NYXHIP_ERR_INVALID_ARG); continue; }
        const uint32_t l = flat ? 0u : bin_pixel(A.inten[R.off + i], R.vmin, R.vmax, g);
        lo = l < lo ? l : lo; hi = l > hi ? l : hi;
    }
    atomicMin(&s_lo, lo); atomicMax(&s_hi, hi);
    __syncthreads();
    if (tid != 0) return;
    lo = s_lo; hi = s_hi;
    if (R.n64 < R.cells) {                                 // cells outside the cloud hold the background level
        const uint32_t bg = g > 0 ? 1u : 0u;
        lo = bg < lo ? bg : lo; hi = bg > hi ? bg : hi;
    }
    // I is 0 .. max in IBSI mode and the distinct levels otherwise (3d_ngtdm.cpp:205-218); fewer than two: soft_nan (:233-241).  With no
    // zone P = N / 0 is NaN in every formula but calc_Busyness, which answers 0 for a single distinct level first (:465)
    const bool few = A.ibsi ? hi == 0u : lo == hi;
    const double nan = __builtin_nan("");
    for (int k = 0; k < kVtNgtdmCols; k++) o[k] = few ? A.soft_nan : (k == 2 && lo == hi) ? 0.0 : nan;
}

// ---- closing ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool vt_present(const uint32_t* pres, uint32_t l) { return (pres[l >> 5] >> (l & 31u)) & 1u; }

// GLDM (3d_gldm.cpp:270-530).  Against the 2-D kernel (roi_dependence.hip): the matrix has 27 dependence columns; Ng is the LARGEST level
// when greyInfo is 0 (:153) with row = level - 1, so absent levels are empty rows of the loops; the entropy adds EPS = 2.2e-16 inside
// fast_log10 and has no p > 0 guard (:419); under matlab binning level 1 is a row that nothing counts into.
__device__ double vt_gldm_feature(int f, const uint32_t* Tm, const int* lv, int Ng, int Nd, double Nz)
{
    auto P = [&](int i, int j) -> double { return (double)(int)Tm[(uint32_t)lv[i - 1] * kVtGldmDeps + (uint32_t)(j - 1)]; };
    double acc = 0.0;
    switch (f) {
    case 0: for (int i = 1; i <= Ng; i++) for (int j = 1; j <= Nd; j++) acc += P(i, j) / ((double)j * (double)j); return acc / Nz;
    case 1: for (int i = 1; i <= Ng; i++) for (int j = 1; j <= Nd; j++) acc += P(i, j) * ((double)j * (double)j); return acc / Nz;
    case 2: for (int i = 1; i <= Ng; i++) { double si = 0.0; for (int j = 1; j <= Nd; j++) si += P(i, j); acc += si * si; } return acc / Nz;
    case 3:
    case 4: for (int j = 1; j <= Nd; j++) { double sj = 0.0; for (int i = 1; i <= Ng; i++) sj += P(i, j); acc += sj * sj; } return f == 3 ? acc / Nz : acc / (Nz * Nz);
    case 5: {
        double mu = 0.0;
        for (int i = 1; i <= Ng; i++) { const double inten = (double)lv[i - 1]; for (int j = 1; j <= Nd; j++) mu += P(i, j) / Nz * inten; }
        for (int i = 1; i <= Ng; i++) { const double inten = (double)lv[i - 1]; for (int j = 1; j <= Nd; j++) { const double mu2 = (inten - mu) * (inten - mu); acc += P(i, j) / Nz * mu2; } }
        return acc;
    }
    case 6: {
        double mu = 0.0;
        for (int i = 1; i <= Ng; i++) for (int j = 1; j <= Nd; j++) mu += P(i, j) / Nz * (double)j;
        for (int i = 1; i <= Ng; i++) for (int j = 1; j <= Nd; j++) { const double dd = (double)j - mu, mu2 = dd * dd; acc += P(i, j) / Nz * mu2; }
        return acc;
    }
    case 7:
        for (int i = 1; i <= Ng; i++) for (int j = 1; j <= Nd; j++) { const double e = fast_log10(P(i, j) / Nz + 2.2e-16) / 0.30102999566; acc += P(i, j) / Nz * e; }
        return -acc;
    case 8: for (int i = 1; i <= Ng; i++) { double i2 = (double)lv[i - 1]; i2 *= i2; double sj = 0.0; for (int j = 1; j <= Nd; j++) sj += P(i, j); acc += sj / i2; } return acc / Nz;
    case 9: for (int i = 1; i <= Ng; i++) { const double inten = (double)lv[i - 1]; double si = 0.0; for (int j = 1; j <= Nd; j++) si += P(i, j); acc += si * inten * inten; } return acc / Nz;
    case 10: for (int i = 1; i <= Ng; i++) { const double inten = (double)lv[i - 1]; for (int j = 1; j <= Nd; j++) acc += P(i, j) / (inten * inten * (double)j * (double)j); } return acc / Nz;
    case 11: for (int i = 1; i <= Ng; i++) { const double inten = (double)lv[i - 1]; for (int j = 1; j <= Nd; j++) acc += P(i, j) * (inten * inten) / (double)(j * j); } return acc / Nz;
    case 12: for (int i = 1; i <= Ng; i++) { const double inten = (double)lv[i - 1]; for (int j = 1; j <= Nd; j++) acc += P(i, j) * (double)(j * j) / (inten * inten); } return acc / Nz;
    default: for (int i = 1; i <= Ng; i++) { const double inten = (double)lv[i - 1]; for (int j = 1; j <= Nd; j++) acc += P(i, j) * (inten * inten * (double)j * (double)j); } return acc / Nz;
    }
}

// NGLDM (3d_ngldm.cpp:259-360), Feature3D order (DCP before GLM).  Against the 2-D kernel: Ns counts column 0 and the loops start at
// column 1; GLV takes the 1-based row index, not the level; nothing guards Ns == 0 (a box without interior cells: 0 / 0).
__device__ double vt_ngldm_feature(int f, const uint32_t* Tm, const int* lv, int Ng, int Nr, double Ns)
{
    auto Sij = [&](int i, int j) -> double { return (double)Tm[(uint32_t)lv[i] * kVtNgldmDeps + (uint32_t)j]; };
    double acc = 0.0;
    if (f == 12) return 1.0;
    if (f == 8 || f == 9) {
        for (int i = 0; i < Ng; i++) { double sj = 0.0; for (int j = 1; j < Nr; j++) sj += Sij(i, j); acc += sj * sj; }
        return f == 8 ? acc / Ns : acc / (Ns * Ns);
    }
    if (f == 10 || f == 11) {
        for (int j = 1; j < Nr; j++) { double sc = 0.0; for (int i = 0; i < Ng; i++) sc += Sij(i, j); acc += sc * sc; }
        return f == 10 ? acc / Ns : acc / (Ns * Ns);
    }
    double mean = 0.0;
    if (f == 14 || f == 16) {
        for (int i = 0; i < Ng; i++) {
            const double iInt = (double)lv[i];
            for (int j = 1; j < Nr; j++) { const double pij = Sij(i, j) / Ns; if (f == 14) mean += iInt * pij; else mean += (double)(j + 1) * pij; }
        }
    }
    for (int i = 0; i < Ng; i++) {
        const double iInt = (double)lv[i], i1 = (double)(i + 1);
        for (int j = 1; j < Nr; j++) {
            const double sij = Sij(i, j), k = (double)(j + 1), pij = sij / Ns;
            switch (f) {
            case 0: acc += sij / j / j; break;
            case 1: acc += sij * j * j; break;
            case 2: if (iInt != 0) acc += sij / iInt / iInt; break;
            case 3: acc += sij * iInt * iInt; break;
            case 4: if (iInt != 0) acc += sij / j / j / iInt / iInt; break;
            case 5: acc += sij * iInt * iInt / k / k; break;
            case 6: if (iInt != 0) acc += sij * k * k / iInt / iInt; break;
            case 7: acc += sij * k * k * iInt * iInt; break;
            case 13: acc += iInt * pij; break;
            case 14: acc += (i1 - mean) * (i1 - mean) * pij; break;
            case 15: acc += (double)(j + 1) * pij; break;
            case 16: acc += (k - mean) * (k - mean) * pij; break;
            case 17: if (pij > 0) acc -= pij * log(pij) / log(2.0); break;
            default: acc += pij * pij; break;
            }
        }
    }
    return f < 8 ? acc / Ns : acc;
}

// NGTDM (3d_ngtdm.cpp:422-536).  Against the 2-D kernel: Ngp is the distinct levels of the whole box; Nvp = Nvc (no average is 0 here);
// nothing guards an empty table (P = 0 / 0).
__device__ double vt_ngtdm_feature(int f, const double* P, const double* S, const int* iv, int Ng, int Ngp, double Nvc)
{
    double sum = 0.0;
    switch (f) {
    case 0: for (int i = 0; i < Ng; i++) sum += P[i] * S[i]; return 1.0 / sum;
    case 1: {
        for (int i = 0; i < Ng; i++) for (int j = 0; j < Ng; j++) { const double a = (double)iv[i], b = (double)iv[j]; sum += P[i] * P[j] * (a - b) * (a - b); }
        const int q = Ngp > 1 ? Ngp * (Ngp - 1) : Ngp;
        const double term1 = sum / (double)q;
        double s2 = 0.0;
        for (int i = 0; i < Ng; i++) s2 += S[i];
        return term1 * (s2 / Nvc);
    }
    case 2: {
        if (Ngp == 1) return 0.0;
        double sum1 = 0.0;
        for (int i = 0; i < Ng; i++) sum1 += P[i] * S[i];
        for (int i = 0; i < Ng; i++) for (int j = 0; j < Ng; j++) if (P[i] != 0 && P[j] != 0) sum += fabs(P[i] * (double)iv[i] - P[j] * (double)iv[j]);
        if (sum == 0) return 0.0;
        return sum1 / sum;
    }
    case 3:
        for (int i = 0; i < Ng; i++) for (int j = 0; j < Ng; j++)
            if (P[i] != 0 && P[j] != 0) sum += fabs((double)iv[i] - (double)iv[j]) * (P[i] * S[i] + P[j] * S[j]) / (P[i] + P[j]);
        return sum / Nvc;
    default: {
        for (int i = 0; i < Ng; i++) for (int j = 0; j < Ng; j++)
            if (P[i] != 0 && P[j] != 0) { const double a = (double)iv[i], b = (double)iv[j]; sum += (P[i] + P[j]) * (a - b) * (a - b); }
        double s2 = 0.0;
        for (int i = 0; i < Ng; i++) s2 += S[i];
        return sum / s2;
    }
    }
}

__global__ __launch_bounds__(64) void voltex_close_kernel(const VoltexArgs A, int n_gldm, int n_ngldm)
{
    __shared__ uint32_t s_T[kVtTabHead + kVtRows * kVtGldmDeps];      // the largest 32-bit table
    __shared__ double s_S[kVtRows], s_P[kVtRows], s_Sc[kVtRows];
    __shared__ int s_lv[kVtRows];
    const int lane = threadIdx.x;
    int f = blockIdx.x, cls = VT_GLDM;
    if (f >= n_gldm) { f -= n_gldm; cls = VT_NGLDM; if (f >= n_ngldm) { f -= n_ngldm; cls = VT_NGTDM; } }
    const VtRoi R = vt_roi(A, blockIdx.y);
    double* const o = A.out + R.roi * A.ld + (cls == VT_GLDM ? A.col_gldm : cls == VT_NGLDM ? A.col_ngldm : A.col_ngtdm) + f;
    if (R.n64 == 0 || R.cells == 0) { if (lane == 0 && R.n64 == 0) *o = A.soft_nan; return; }
    if (!vt_box_fits(A, R)) return;                        // (a binning kernel raised the status)
    if (cls != VT_NGTDM && R.vmin == R.vmax) { if (lane == 0) *o = A.soft_nan; return; }   // 3d_gldm.cpp:61, 3d_ngldm.cpp:173
    const uint32_t* const G = A.tab[cls] + (uint64_t)blockIdx.y * A.tab_stride[cls];
    const uint32_t w32 = cls == VT_GLDM ? kVtGldmWords : cls == VT_NGLDM ? kVtNgldmWords : kVtNgtdmSums;
    for (uint32_t i = lane; i < w32; i += 64u) s_T[i] = G[i];
    if (cls == VT_NGTDM) {
        // S[level] = sum over the classes, in class order, of (exact integer sum) / nd (3d_ngtdm.cpp:115, :164)
        const int r = A.radius;
        const uint32_t ncls = vt_classes(r);
        const unsigned long long* const GS = (const unsigned long long*)(G + kVtNgtdmSums);
        const int mx = ((int)R.w - 1 < r ? (int)R.w - 1 : r) + 1, my = ((int)R.h - 1 < r ? (int)R.h - 1 : r) + 1, mz = ((int)R.d - 1 < r ? (int)R.d - 1 : r) + 1;
        for (uint32_t l = lane; l < kVtRows; l += 64u) {
            double s = 0.0;
            for (uint32_t k = 0; k < ncls; k++) {
                const unsigned long long v = GS[l * ncls + k];
                if (v == 0ull) continue;
                const int ax = (int)(k % (uint32_t)(r + 1)), ay = (int)(k / (uint32_t)(r + 1)) % (r + 1), az = (int)(k / (uint32_t)((r + 1) * (r + 1)));
                const int nd = (mx + ax) * (my + ay) * (mz + az) - 1;
                s += (double)v / (double)nd;
            }
            s_Sc[l] = s;
        }
    }
    __syncthreads();
    if (lane != 0) return;
    const uint32_t* const pres = s_T;
    const uint32_t* const Tm = s_T + kVtTabHead;
    int top = -1, npres = 0;
    for (uint32_t l = 0; l < kVtRows; l++) if (vt_present(pres, l)) { top = (int)l; npres++; }
    if (cls == VT_GLDM) {
        const int g = A.g_gldm;
        int Ng = 0;
        if (g == 0) { for (int l = 1; l <= top; l++) s_lv[Ng++] = l; }                       // I = 1 .. max (:100-107)
        else { for (uint32_t l = 1; l < kVtRows; l++) if (vt_present(pres, l)) s_lv[Ng++] = (int)l; }   // the distinct levels but 0 (:110-113)
        uint32_t Nz = 0; int maxNd = 0;
        for (uint32_t l = 0; l < kVtRows; l++) for (uint32_t j = 0; j < kVtGldmDeps; j++) { const uint32_t c = Tm[l * kVtGldmDeps + j]; Nz += c; if (c && (int)j + 1 > maxNd) maxNd = (int)j + 1; }
        if (Nz == 0 || Ng == 0) { *o = A.soft_nan; return; }                                 // :196-213
        *o = vt_gldm_feature(f, Tm, s_lv, Ng, g ? maxNd : (int)kVtGldmDeps, (double)Nz);
    } else if (cls == VT_NGLDM) {
        int Ng = 0;
        for (uint32_t l = 0; l < kVtRows; l++) if (vt_present(pres, l)) s_lv[Ng++] = (int)l;  // the distinct levels, 0 too (:88-101)
        double Ns = 0.0; int maxdep = 0;
        for (uint32_t l = 0; l < kVtRows; l++) for (uint32_t j = 0; j < kVtNgldmDeps; j++) if (Tm[l * kVtNgldmDeps + j] && (int)j > maxdep) maxdep = (int)j;
        const int Nr = maxdep + 1;                                                            // :165
        for (int i = 0; i < Ng; i++) for (int j = 0; j < Nr; j++) Ns += (double)Tm[(uint32_t)s_lv[i] * kVtNgldmDeps + (uint32_t)j];
        *o = vt_ngldm_feature(f, Tm, s_lv, Ng, Nr, Ns);
    } else {
        // I: 0 .. max in IBSI mode, the distinct levels otherwise; 1 is added to every level when the smallest is 0 (:205-227)
        const bool shift = A.ibsi || vt_present(pres, 0u);
        int Ng = 0;
        double Nvc = 0.0;
        for (int l = 0; l <= top; l++) {
            if (!A.ibsi && !vt_present(pres, (uint32_t)l)) continue;
            s_lv[Ng] = l + (shift ? 1 : 0);
            s_P[Ng] = (double)Tm[l];                       // N[row], for now
            s_S[Ng] = s_Sc[l];
            Nvc += (double)Tm[l];
            Ng++;
        }
        if (Ng < 2) { *o = A.soft_nan; return; }                                              // :233-241
        for (int i = 0; i < Ng; i++) s_P[i] = s_P[i] / Nvc;
        *o = vt_ngtdm_feature(f, s_P, s_S, s_lv, Ng, npres, Nvc);
    }
}

} // namespace

int launch_voltex_bin_ngldm(const VoltexArgs& a, uint32_t max_px, void* stream)
{
    if (a.n_roi == 0) return 0;
    uint32_t gx = (max_px + 2047u) / 2048u;
    gx = gx < 1u ? 1u : gx > 256u ? 256u : gx;
    hipLaunchKernelGGL(voltex_bin_ngldm_kernel, dim3(gx, (uint32_t)a.n_roi), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_voltex_sweep(const VoltexArgs& a, int cls, void* stream)
{
    if (a.n_roi == 0) return 0;
    const dim3 grid((a.max_cells + kVtCellsPerWg - 1u) / kVtCellsPerWg, (uint32_t)a.n_roi);
    if (cls == VT_GLDM) hipLaunchKernelGGL(voltex_sweep_kernel<VT_GLDM>, grid, dim3(256), 4u * kVtGldmWords, (hipStream_t)stream, a);
    else if (cls == VT_NGLDM) hipLaunchKernelGGL(voltex_sweep_kernel<VT_NGLDM>, grid, dim3(256), 4u * kVtNgldmWords, (hipStream_t)stream, a);
    else {
        static DeviceOnce optin;
        if (int orc = optin.run([]() -> int {
                return (int)hipFuncSetAttribute((const void*)voltex_sweep_kernel<VT_NGTDM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)(4u * vt_ngtdm_words(kVtMaxRadius)));
            }))
            return orc;
        hipLaunchKernelGGL(voltex_sweep_kernel<VT_NGTDM>, grid, dim3(256), 4u * vt_ngtdm_words(a.radius), (hipStream_t)stream, a);
    }
    return (int)hipGetLastError();
}

int launch_voltex_ngtdm_r0(const VoltexArgs& a, void* stream)
{
    if (a.n_roi == 0) return 0;
    hipLaunchKernelGGL(voltex_ngtdm_r0_kernel, dim3((uint32_t)a.n_roi), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_voltex_close(const VoltexArgs& a, void* stream)
{
    const int ng = a.col_gldm >= 0 ? kVtGldmCols : 0, nn = a.col_ngldm >= 0 ? kVtNgldmCols : 0, nt = a.col_ngtdm >= 0 && a.radius > 0 ? kVtNgtdmCols : 0;
    if (a.n_roi == 0 || ng + nn + nt == 0) return 0;
    hipLaunchKernelGGL(voltex_close_kernel, dim3((uint32_t)(ng + nn + nt), (uint32_t)a.n_roi), dim3(64), 0, (hipStream_t)stream, a, ng, nn);
    return (int)hipGetLastError();
}

} // namespace nyxhip
