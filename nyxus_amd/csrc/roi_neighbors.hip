// roi_neighbors.hip -- NeighborsFeature (features/neighbors.cpp:125-536 of the reference, its single-thread branch): the one class of the
// shape block that relates the ROIs of an image to each other.  Reads the merged contours roi_contour_kernel left in the workspace.
//
//   nb_geometry_kernel      a wave per ROI: the box in image coordinates (i64), the centroid from u64 sums (the scheme of roi_circle.hip:
//                           basic_morphology.cpp:40-47, exact below 2^53), the rows [lo, hi) of the ROI's image; checks that labels ascend.
//   nb_count / scan / fill  per ROI the rows j != i of its image whose boxes overlap at the radius (aabbNoOverlap, neighbors.cpp:539-547,
//                           in 64-bit integers) and whose contours -- like its own -- are not empty (:261), ascending: count, exclusive
//                           scan, fill.  The layout is a function of the input alone (no atomics-ordered append).
//   roi_neighbors_narrow_kernel   THE HOT PATH.  A workgroup per ROI i loops over its candidates j.  K_i lies across the lanes, kNbPointsPerLane
//                           points a lane (longer contours: several passes); K_j is moved into i's frame, streamed through LDS in tiles
//                           of kNbTile points and read as broadcasts.  Every lane keeps min_j sqdist(K_i[p], K_j[.]) of its points as
//                           exact integers (32 bits when the pair's extent allows, 64 otherwise); its touch flags (d <= 2, BEFORE the radius gate, per contour
//                           INDEX, :268-280) stay private; a workgroup reduction gives the pair's `mind`, which is symmetric -- so the
//                           directed form (i -> j here, j -> i in j's workgroup) makes the reference's decisions.  No atomics.
//                           Writes NUM_NEIGHBORS, PERCENT_TOUCHING and the per-candidate neighbor flag.
//   nb_close_kernel         a lane per ROI over its flagged candidates in ascending row (= label) order, the order of the reference's
//                           aux_neighboring_labels: the two first minima of the centroid distances, their angles, the Welford recurrence
//                           of Moments2 (moments.h:15-38) and the mode of the rounded angles.  fp64, unfused (-ffp-contract=off), IEEE
//                           division and square root.
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "roi_neighbors.h"
#include "../../include/nyxhip.h"

namespace nyxhip {

namespace {

constexpr int kGeoWaves = 4;               // ROIs (waves) per workgroup of nb_geometry_kernel
constexpr int kScanThreads = 1024;

__device__ __forceinline__ bool nb_overlap(const long long* box, uint64_t a, uint64_t b, long long R)
{
    const long long xmin1 = box[4 * a], xmax1 = box[4 * a + 1], ymin1 = box[4 * a + 2], ymax1 = box[4 * a + 3];
    const long long xmin2 = box[4 * b], xmax2 = box[4 * b + 1], ymin2 = box[4 * b + 2], ymax2 = box[4 * b + 3];
    const bool no = xmin2 - R > xmax1 + R || xmax2 + R < xmin1 - R || ymin2 - R > ymax1 + R || ymax2 + R < ymin1 - R;
    return !no;
}

template <typename D> __device__ __forceinline__ D nb_sq(int d);
template <> __device__ __forceinline__ uint32_t nb_sq<uint32_t>(int d) { return (uint32_t)__mul24(d, d); }                     // |d| <= 46340
template <> __device__ __forceinline__ unsigned long long nb_sq<unsigned long long>(int d) { return (unsigned long long)((long long)d * (long long)d); }

// One candidate against the points a lane holds: min over K_j per point, then the lane's touch bits and minimum.
template <typename D>
__device__ __forceinline__ unsigned long long nb_pair(int2* s_K, const uint32_t* Kj, uint32_t nKj, int ddx, int ddy, const int (&xi)[kNbPointsPerLane],
                                                      const int (&yi)[kNbPointsPerLane], uint32_t vmask, int pcount, uint32_t& tmask, int tid)
{
    D m[kNbPointsPerLane];
#pragma unroll
    for (int p = 0; p < kNbPointsPerLane; p++) m[p] = ~(D)0;
    for (uint32_t t0 = 0; t0 < nKj; t0 += (uint32_t)kNbTile) {
        const int cnt = (int)min((uint32_t)kNbTile, nKj - t0);
        __syncthreads();                                                      // the previous tile has been read by every wave
        for (int q = tid; q < cnt; q += kNbThreads) {
            const uint32_t k = Kj[t0 + (uint32_t)q];
            s_K[q] = make_int2((int)(k & 0xFFFFu) + ddx, (int)(k >> 16) + ddy);
        }
        __syncthreads();
        if (pcount > 0) {                                                     // (wave-uniform: a wave without points of this pass only keeps the barriers)
#pragma unroll 4
            for (int q = 0; q < cnt; q++) {
                const int2 pj = s_K[q];                                       // one address per wave: a broadcast
#pragma unroll
                for (int p = 0; p < kNbPointsPerLane; p++)
                    if (p < pcount) {
                        const D d = nb_sq<D>(xi[p] - pj.x) + nb_sq<D>(yi[p] - pj.y);
                        m[p] = d < m[p] ? d : m[p];
                    }
            }
        }
    }
    unsigned long long lm = ~0ull;
#pragma unroll
    for (int p = 0; p < kNbPointsPerLane; p++)
        if ((vmask >> p) & 1u) {
            if (m[p] <= (D)2) tmask |= 1u << p;                               // touchThresh2 (neighbors.cpp:243)
            lm = (unsigned long long)m[p] < lm ? (unsigned long long)m[p] : lm;
        }
    return lm;
}

} // namespace

__global__ void nb_extrema_kernel(uint64_t n_roi, const uint64_t* px_offset, const uint32_t* bw, const uint32_t* bh, uint32_t* ext3)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n_roi) return;
    const uint64_t n = px_offset[i + 1] - px_offset[i], a = (uint64_t)bw[i] * bh[i];
    atomicMax(&ext3[0], (uint32_t)min(n, (uint64_t)0xFFFFFFFFu));
    atomicMax(&ext3[1], (uint32_t)min(a, (uint64_t)0xFFFFFFFFu));
    atomicMax(&ext3[2], max(bw[i], bh[i]));
}

__global__ __launch_bounds__(64 * kGeoWaves) void nb_geometry_kernel(const NbArgs A)
{
    const int lane = threadIdx.x & 63;
    const uint64_t roi = (uint64_t)blockIdx.x * kGeoWaves + (uint64_t)(threadIdx.x >> 6);
    if (roi >= A.n_roi)
        return;
    const uint64_t off = A.px_offset[roi];
    const uint32_t n = (uint32_t)(A.px_offset[roi + 1] - off);
    unsigned long long sx = 0, sy = 0;
    for (uint32_t i = (uint32_t)lane; i < n; i += 64) { sx += A.x[off + i]; sy += A.y[off + i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); }
    if (lane != 0)
        return;
    const unsigned long long ox = A.origin_x ? A.origin_x[roi] : 0, oy = A.origin_y ? A.origin_y[roi] : 0;
    A.box[4 * roi] = (long long)ox;
    A.box[4 * roi + 1] = (long long)ox + (long long)A.bbox_w[roi] - 1;
    A.box[4 * roi + 2] = (long long)oy;
    A.box[4 * roi + 3] = (long long)oy + (long long)A.bbox_h[roi] - 1;
    A.cen[2 * roi] = n ? (double)(sx + (unsigned long long)n * ox) / (double)n : 0.0;     // basic_morphology.cpp:40-47
    A.cen[2 * roi + 1] = n ? (double)(sy + (unsigned long long)n * oy) / (double)n : 0.0;
    uint64_t lo = 0, hi = A.n_roi;
    if (A.image_offset) {                                                     // the last image k with image_offset[k] <= roi
        uint64_t a = 0, b = A.n_images;                                       // invariant: image_offset[a] <= roi, the answer lies in [a, b)
        while (b - a > 1) {
            const uint64_t mid = a + (b - a) / 2;
            if (A.image_offset[mid] <= roi) a = mid; else b = mid;
        }
        lo = min(A.image_offset[a], roi);
        hi = max(min(A.image_offset[a + 1], A.n_roi), roi + 1);
    } else if (A.image_id) {
        const uint32_t id = A.image_id[roi];
        uint64_t a = 0, b = roi;                                              // first row of this image
        while (a < b) { const uint64_t mid = a + (b - a) / 2; if (A.image_id[mid] < id) a = mid + 1; else b = mid; }
        lo = a;
        a = roi + 1; b = A.n_roi;                                             // first row behind it
        while (a < b) { const uint64_t mid = a + (b - a) / 2; if (A.image_id[mid] <= id) a = mid + 1; else b = mid; }
        hi = a;
    }
    A.img_lo[roi] = (uint32_t)lo;
    A.img_hi[roi] = (uint32_t)hi;
    if (roi > lo && A.label[roi] <= A.label[roi - 1])
        atomicCAS(A.status, 0, NYXHIP_ERR_INVALID_ARG);                       // rows of an image must ascend strictly in roi_label
}

template <bool FILL>
__global__ void nb_candidates_kernel(const NbArgs A)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= A.n_roi) return;
    uint32_t k = 0;
    uint32_t* const dst = FILL ? A.cand + A.cand_off[i] : nullptr;
    if (A.n_contour[i] != 0) {
        const uint32_t lo = A.img_lo[i], hi = A.img_hi[i];
        for (uint32_t j = lo; j < hi; j++)
            if (j != (uint32_t)i && A.n_contour[j] != 0 && nb_overlap(A.box, i, j, A.radius)) {
                if (FILL) dst[k] = j;
                k++;
            }
    }
    if (!FILL) A.cand_count[i] = k;
}

// exclusive scan of cand_count into cand_off (one workgroup walks the array; cand_off[n_roi] is the total)
__global__ __launch_bounds__(kScanThreads) void nb_scan_kernel(const uint32_t* cnt, uint64_t* off, uint64_t n)
{
    __shared__ unsigned long long s_w[kScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n; base += kScanThreads) {
        const uint64_t i = base + (uint64_t)tid;
        const unsigned long long v = i < n ? cnt[i] : 0;
        unsigned long long inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        __syncthreads();                                                      // s_w of the previous round has been read
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        unsigned long long before = 0, total = 0;
        for (int w = 0; w < kScanThreads / 64; w++) {
            const unsigned long long t = s_w[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < n) off[i] = carry + before + inc - v;
        carry += total;
    }
    if (tid == 0) off[n] = carry;
}

__global__ __launch_bounds__(kNbThreads) void roi_neighbors_narrow_kernel(const NbArgs A)
{
    __shared__ int2 s_K[kNbTile];
    __shared__ unsigned long long s_red[kNbThreads / 64];
    __shared__ uint32_t s_cnt[2 * (kNbThreads / 64)];
    const uint64_t i = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* const row_out = A.out + i * A.ld;
    const uint32_t nKi = A.n_contour[i];
    const uint64_t c0 = A.cand_off[i];
    const uint32_t nc = (uint32_t)(A.cand_off[i + 1] - c0);
    if (nc == 0 || nKi == 0) {                                                // no candidate (an empty contour has none): the zeros of the reference
        if (tid < 2) row_out[tid] = 0.0;
        return;
    }
    const uint32_t* const Ki = A.ws_contour + A.px_offset[i];
    const long long oxi = A.origin_x ? (long long)A.origin_x[i] : 0, oyi = A.origin_y ? (long long)A.origin_y[i] : 0;
    const int wi = (int)max(A.bbox_w[i], A.bbox_h[i]);
    uint32_t touched = 0;
    for (uint32_t pbase = 0; pbase < nKi; pbase += (uint32_t)(kNbThreads * kNbPointsPerLane)) {
        int xi[kNbPointsPerLane], yi[kNbPointsPerLane];
        uint32_t vmask = 0;
        int pcount = 0;                                                       // points of this pass the WAVE holds (uniform)
#pragma unroll
        for (int p = 0; p < kNbPointsPerLane; p++) {
            const uint32_t idx = pbase + (uint32_t)(p * kNbThreads + tid);
            if (pbase + (uint32_t)(p * kNbThreads + wave * 64) < nKi) pcount = p + 1;
            if (idx < nKi) vmask |= 1u << p;
            const uint32_t k = Ki[idx < nKi ? idx : nKi - 1];                 // (a lane without a point repeats the last one; vmask keeps it out)
            xi[p] = (int)(k & 0xFFFFu);
            yi[p] = (int)(k >> 16);
        }
        uint32_t tmask = 0;
        for (uint32_t c = 0; c < nc; c++) {
            const uint32_t j = A.cand[c0 + c];
            const uint32_t nKj = A.n_contour[j];
            const uint32_t* const Kj = A.ws_contour + A.px_offset[j];
            const long long dxl = (A.origin_x ? (long long)A.origin_x[j] : 0) - oxi, dyl = (A.origin_y ? (long long)A.origin_y[j] : 0) - oyi;
            const int ddx = (int)dxl, ddy = (int)dyl;                         // (boxes that overlap at the radius: |d| < 2^16 + 2 * kNbMaxDistance)
            const int wj = (int)max(A.bbox_w[j], A.bbox_h[j]);
            const int ext = max(abs(ddx), abs(ddy)) + max(wi, wj) + 2;         // bound of |dx|, |dy| over the pair's points
            unsigned long long lm;
            if (ext <= 46340)                                                 // dx * dx + dy * dy < 2^32
                lm = nb_pair<uint32_t>(s_K, Kj, nKj, ddx, ddy, xi, yi, vmask, pcount, tmask, tid);
            else
                lm = nb_pair<unsigned long long>(s_K, Kj, nKj, ddx, ddy, xi, yi, vmask, pcount, tmask, tid);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(lm, o, 64); lm = t < lm ? t : lm; }
            if (lane == 0) s_red[wave] = lm;
            __syncthreads();
            if ((int)(c & (uint32_t)(kNbThreads - 1)) == tid) {               // candidate c is kept by lane c mod kNbThreads, here and below
                unsigned long long mn = s_red[0];
#pragma unroll
                for (int w = 1; w < kNbThreads / 64; w++) mn = s_red[w] < mn ? s_red[w] : mn;
                if (pbase != 0) { const unsigned long long old = A.cand_min[c0 + c]; mn = old < mn ? old : mn; }
                A.cand_min[c0 + c] = mn;
            }
            // (s_red is written again behind the two barriers of the next nb_pair)
        }
        touched += (uint32_t)__popc(tmask);
    }
    const unsigned long long r2 = (unsigned long long)(A.radius * A.radius);
    uint32_t nn = 0;
    for (uint32_t c = (uint32_t)tid; c < nc; c += (uint32_t)kNbThreads) {
        const uint8_t f = A.cand_min[c0 + c] <= r2 ? 1 : 0;                   // `mind > radius2`: not a neighbor (neighbors.cpp:283)
        A.cand_flag[c0 + c] = f;
        nn += f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { touched += __shfl_xor(touched, o, 64); nn += __shfl_xor(nn, o, 64); }
    if (lane == 0) { s_cnt[2 * wave] = touched; s_cnt[2 * wave + 1] = nn; }
    __syncthreads();
    if (tid == 0) {
        uint32_t nt = 0, nb = 0;
        for (int w = 0; w < kNbThreads / 64; w++) { nt += s_cnt[2 * w]; nb += s_cnt[2 * w + 1]; }
        row_out[0] = (double)nb;
        row_out[1] = 100.0 * (double)nt / (double)nKi;                        // neighbors.cpp:306
    }
}

__global__ void nb_close_kernel(const NbArgs A)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= A.n_roi) return;
    double* const row_out = A.out + i * A.ld;
    double v[7] = {0, 0, 0, 0, 0, 0, 0};                                      // CLOSEST_NEIGHBOR1_DIST .. ANG_BW_NEIGHBORS_MODE
    const uint64_t c0 = A.cand_off[i], c1 = A.cand_off[i + 1];
    const double cx = A.cen[2 * i], cy = A.cen[2 * i + 1];
    // direction_angle_deg (neighbors.cpp:21-27); atan2(0, 0) is taken as 0
    auto angle_to = [&](uint32_t j) -> double {
        const double dy = A.cen[2 * (uint64_t)j + 1] - cy, dx = A.cen[2 * (uint64_t)j] - cx;
        double ang = (dy == 0.0 && dx == 0.0) ? 0.0 : atan2(dy, dx) * 180.0 / 3.14159265358979323846;
        if (ang < 0.0) ang += 360.0;
        return ang;
    };
    auto dist_to = [&](uint32_t j) -> double {
        const double dx = cx - A.cen[2 * (uint64_t)j], dy = cy - A.cen[2 * (uint64_t)j + 1];
        return sqrt(dx * dx + dy * dy);
    };
    // pass 1: the first minimum, the Welford recurrence (Moments2::add) and the rounded angles
    uint64_t n = 0, k1 = 0;
    double d1 = 0.0, mean = 0.0, M2 = 0.0;
    for (uint64_t c = c0; c < c1; c++) {
        if (!A.cand_flag[c]) continue;
        const uint32_t j = A.cand[c];
        const double d = dist_to(j), ang = angle_to(j);
        if (n == 0 || d < d1) { d1 = d; k1 = c; }
        const uint64_t n1 = n;
        n = n + 1;
        const double delta = ang - mean, delta_n = delta / (double)n, term1 = delta * delta_n * (double)n1;
        mean = mean + delta_n;
        M2 += term1;
        int ra = (int)round(ang);
        ra = max(0, min(360, ra));
        A.cand_ang[c] = (uint16_t)ra;
    }
    if (n != 0) {
        v[0] = d1;
        v[1] = angle_to(A.cand[k1]);
        if (n > 1) {                                                          // the first minimum of the rest (neighbors.cpp:478-491)
            bool have = false;
            uint64_t k2 = 0;
            double d2 = 0.0;
            for (uint64_t c = c0; c < c1; c++) {
                if (!A.cand_flag[c] || c == k1) continue;
                const double d = dist_to(A.cand[c]);
                if (!have || d < d2) { d2 = d; k2 = c; have = true; }
            }
            v[2] = d2;
            v[3] = angle_to(A.cand[k2]);
        }
        v[4] = mean;
        v[5] = n > 2 ? sqrt(M2 / (double)(n - 1)) : 0.0;
        // the smallest rounded angle among those with the highest count (neighbors.cpp:522-531)
        int mode = 0, mode_cnt = 0;
        for (uint64_t c = c0; c < c1; c++) {
            if (!A.cand_flag[c]) continue;
            const int a = A.cand_ang[c];
            int cnt = 0;
            for (uint64_t e = c0; e < c1; e++) cnt += (A.cand_flag[e] && A.cand_ang[e] == a) ? 1 : 0;
            if (cnt > mode_cnt || (cnt == mode_cnt && a < mode)) { mode_cnt = cnt; mode = a; }
        }
        v[6] = (double)mode;
    }
#pragma unroll
    for (int k = 0; k < 7; k++) row_out[2 + k] = v[k];
}

int launch_nb_extrema(uint64_t n_roi, const uint64_t* px_offset, const uint32_t* bw, const uint32_t* bh, uint32_t* ext3, void* stream)
{
    hipLaunchKernelGGL(nb_extrema_kernel, dim3((unsigned)((n_roi + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_roi, px_offset, bw, bh, ext3);
    return (int)hipGetLastError();
}

int launch_nb_geometry(const NbArgs& a, void* stream)
{
    hipLaunchKernelGGL(nb_geometry_kernel, dim3((unsigned)((a.n_roi + kGeoWaves - 1) / kGeoWaves)), dim3(64 * kGeoWaves), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_nb_candidates_count(const NbArgs& a, void* stream)
{
    hipLaunchKernelGGL(nb_candidates_kernel<false>, dim3((unsigned)((a.n_roi + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(nb_scan_kernel, dim3(1), dim3(kScanThreads), 0, (hipStream_t)stream, (const uint32_t*)a.cand_count, a.cand_off, a.n_roi);
    return (int)hipGetLastError();
}

int launch_nb_candidates_fill(const NbArgs& a, void* stream)
{
    hipLaunchKernelGGL(nb_candidates_kernel<true>, dim3((unsigned)((a.n_roi + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_nb_narrow(const NbArgs& a, void* stream)
{
    hipLaunchKernelGGL(roi_neighbors_narrow_kernel, dim3((unsigned)a.n_roi), dim3(kNbThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_nb_close(const NbArgs& a, void* stream)
{
    hipLaunchKernelGGL(nb_close_kernel, dim3((unsigned)((a.n_roi + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace nyxhip
