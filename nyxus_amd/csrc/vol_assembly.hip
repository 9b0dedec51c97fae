// vol_assembly.hip -- the label scan of nyxhip_assemble_volumes on the device: a stack of intensity / label volumes resident in HBM ->
// the rows and voxel clouds of a nyxhip_batch3d, bit for bit what clouds_from_volume + batch3d_from_rois (nyxus_amd) assemble on the host.
// The shape of tile_assembly.hip with a z axis; label VALUES are arbitrary 32-bit numbers, nothing is sized by the label magnitude.
//   vol_scan_kernel      one coalesced pass over the volumes in kVsScanCols x kVsScanRows blocks of ONE z-plane; a thread walks a column
//                        segment and keeps the run of its current label in registers, runs merge in an LDS hash table keyed by label, and
//                        only the live LDS entries reach the volume's open-addressing table in HBM (count, vmin, vmax, min / max of x, y, z).
//                        An insertion that finds no slot raises VS_META_STATUS: the host replaces the tables by larger ones and scans again.
//   vs_count / vs_compact   occupied slots -> rows in slot order (any order: the sort below places them), per 1024-entry block.
//   vs_sort_*            ascending (volume, label) order by an LSD radix sort of 64-bit keys, 8 bits a pass, stable through ballot ranks:
//                        per pass a digit count per kVsSortTile keys, one prefix sum, one scatter.  Linear in the rows (volscan_plan.h);
//                        the counting rank of tile_rank_kernel is quadratic in the labels of a tile and does not carry over to the
//                        10^4 .. 10^5 labels of a 3-D cell segmentation.
//   vs_gather / vs_offsets  the sorted rows, their z-slabs, the stated extrema of the batch, CSR offsets by prefix sums.
//   vol_cloud_kernel     one workgroup per (ROI, slab of z-planes) reads its part of the ROI's box window in raster order (z, y, x) and
//                        writes x / y / z / inten by the ballot-ranked compaction of roi_cloud_kernel.  A box of at most kVsSlabCells
//                        cells is one slab: one workgroup, no count pass.  A larger box is cut into slabs: a count pass (hits per slab),
//                        the prefix over the slabs in front of mine, then the write pass.  A position never depends on which wave or
//                        workgroup arrives first: CSR offset + hits of the slabs in front + ballot rank.
//                        COST: the launch reads the sum of the BOX volumes, not of the ROI volumes: a label scattered over the whole
//                        volume re-reads the volume (twice when its box takes the slab form), and n such labels read it n times.
// Volumes keep the caller's element types (8 / 16 / 32-bit unsigned): the scan and the cloud kernels are instantiated per type pair.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "volscan_plan.h"

namespace nyxhip {

namespace {

__device__ __forceinline__ uint32_t vs_mix(uint32_t l)
{
    l ^= l >> 16; l *= 0x85EBCA6Bu; l ^= l >> 13; l *= 0xC2B2AE35u; l ^= l >> 16;
    return l;
}

__device__ __forceinline__ uint32_t vs_wave_max(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}

__device__ __forceinline__ unsigned long long vs_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Exclusive prefix sum of v over the workgroup's threads (blockDim.x a multiple of 64, at most 1024) and the workgroup's total.
// s_w: 16 words of LDS, free again when the call returns.
__device__ __forceinline__ unsigned long long vs_block_scan(unsigned long long v, unsigned long long* s_w, unsigned long long* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
    for (int w = 0; w < nw; w++) { const unsigned long long c = s_w[w]; if (w < wave) base += c; tot += c; }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

__global__ void vs_init_kernel(VsTable T, uint64_t n)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < n) {
        T.key[i] = 0; T.cnt[i] = 0; T.vmin[i] = 0xFFFFFFFFu; T.vmax[i] = 0;
        T.xmin[i] = 0xFFFFFFFFu; T.xmax[i] = 0; T.ymin[i] = 0xFFFFFFFFu; T.ymax[i] = 0; T.zmin[i] = 0xFFFFFFFFu; T.zmax[i] = 0;
    }
}

// One workgroup owns a kVsScanCols x kVsScanRows block of a z-plane (and of every kVsMaxPlanesGrid-th plane behind it); a thread walks one
// column of the block.  The LDS table needs no z: a block lies in one plane.
template <typename TI, typename TL>
__global__ __launch_bounds__(kVsScanCols) void vol_scan_kernel(const TI* __restrict__ inten, const TL* __restrict__ label, uint32_t W, uint32_t H, uint32_t D,
                                                               uint32_t n_planes, VsTable T, uint32_t* meta)
{
    __shared__ uint32_t s_key[kVsLdsCap], s_cnt[kVsLdsCap], s_vmin[kVsLdsCap], s_vmax[kVsLdsCap], s_xmin[kVsLdsCap], s_xmax[kVsLdsCap],
        s_ymin[kVsLdsCap], s_ymax[kVsLdsCap];
    const int tid = threadIdx.x;
    const uint32_t x = blockIdx.x * kVsScanCols + tid;
    const uint32_t y_begin = blockIdx.y * kVsScanRows;
    const uint32_t y_end = y_begin + kVsScanRows < H ? y_begin + kVsScanRows : H;
    const uint32_t capm = T.cap - 1;

    for (uint32_t plane = blockIdx.z; plane < n_planes; plane += gridDim.z) {
        for (int i = tid; i < kVsLdsCap; i += kVsScanCols) {
            s_key[i] = 0; s_cnt[i] = 0; s_vmin[i] = 0xFFFFFFFFu; s_vmax[i] = 0;
            s_xmin[i] = 0xFFFFFFFFu; s_xmax[i] = 0; s_ymin[i] = 0xFFFFFFFFu; s_ymax[i] = 0;
        }
        __syncthreads();
        const uint32_t vol = plane / D, z = plane - vol * D;
        const uint64_t tbase = (uint64_t)vol * T.cap;

        // one run (or one LDS entry) into the volume's table: linear probing, the slot is claimed by CAS on the label
        auto to_global = [&](uint32_t l, uint32_t cnt, uint32_t mn, uint32_t mx, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1) {
            if (__hip_atomic_load(&meta[VS_META_STATUS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)
                return;                                      // the scan is void already: the host scans again with larger tables
            uint32_t h = vs_mix(l) & capm;
            for (uint32_t probe = 0; probe < T.probes; probe++) {
                const uint64_t g = tbase + h;
                const uint32_t prev = atomicCAS(&T.key[g], 0u, l);
                if (prev == 0u || prev == l) {
                    atomicAdd(&T.cnt[g], cnt);
                    atomicMin(&T.vmin[g], mn); atomicMax(&T.vmax[g], mx);
                    atomicMin(&T.xmin[g], x0); atomicMax(&T.xmax[g], x1);
                    atomicMin(&T.ymin[g], y0); atomicMax(&T.ymax[g], y1);
                    atomicMin(&T.zmin[g], z); atomicMax(&T.zmax[g], z);
                    return;
                }
                h = (h + 1) & capm;
            }
            atomicMax(&meta[VS_META_STATUS], 1u);
        };
        auto flush = [&](uint32_t l, uint32_t cnt, uint32_t mn, uint32_t mx, uint32_t y0, uint32_t y1) {
            uint32_t h = vs_mix(l) & (kVsLdsCap - 1);
            for (int probe = 0; probe < kVsLdsProbes; probe++) {
                const uint32_t prev = atomicCAS(&s_key[h], 0u, l);
                if (prev == 0u || prev == l) {
                    atomicAdd(&s_cnt[h], cnt);
                    atomicMin(&s_vmin[h], mn); atomicMax(&s_vmax[h], mx);
                    atomicMin(&s_xmin[h], x); atomicMax(&s_xmax[h], x);
                    atomicMin(&s_ymin[h], y0); atomicMax(&s_ymax[h], y1);
                    return;
                }
                h = (h + 1) & (kVsLdsCap - 1);
            }
            to_global(l, cnt, mn, mx, x, x, y0, y1);         // block table crowded (label confetti): straight to the volume's table
        };

        if (x < W) {
            const uint64_t col = ((uint64_t)plane * H) * W + x;
            uint32_t cur = 0, cnt = 0, mn = 0xFFFFFFFFu, mx = 0, y0 = 0, y1 = 0;
            constexpr int kB = kVsScanBatch;
            for (uint32_t yb = y_begin; yb < y_end; yb += kB) {
                uint32_t l[kB], v[kB];
#pragma unroll
                for (int k = 0; k < kB; k++) {               // all loads of the batch in flight before first use
                    const uint32_t y = yb + k;
                    const bool in = y < y_end;
                    l[k] = in ? (uint32_t)label[col + (uint64_t)y * W] : 0u;
                    v[k] = in ? (uint32_t)inten[col + (uint64_t)y * W] : 0u;
                }
#pragma unroll
                for (int k = 0; k < kB; k++) {
                    const uint32_t y = yb + k;
                    if (l[k] != cur) {
                        if (cur) flush(cur, cnt, mn, mx, y0, y1);
                        cur = l[k]; cnt = 0; mn = 0xFFFFFFFFu; mx = 0; y0 = y;
                    }
                    if (cur) { cnt++; mn = v[k] < mn ? v[k] : mn; mx = v[k] > mx ? v[k] : mx; y1 = y; }
                }
            }
            if (cur) flush(cur, cnt, mn, mx, y0, y1);
        }
        __syncthreads();
        for (int i = tid; i < kVsLdsCap; i += kVsScanCols) {
            const uint32_t l = s_key[i];
            if (l == 0) continue;
            to_global(l, s_cnt[i], s_vmin[i], s_vmax[i], s_xmin[i], s_xmax[i], s_ymin[i], s_ymax[i]);
        }
        __syncthreads();                                     // the table is cleared for the next plane only when every entry has left it
    }
}

__global__ __launch_bounds__(kVsScanThreads) void vs_count_kernel(VsTable T, uint64_t n_entries, uint32_t* blk_rows, uint32_t* meta)
{
    __shared__ uint32_t s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t e = blockIdx.x * (uint64_t)kVsScanThreads + tid;
    const bool occ = e < n_entries && T.key[e] != 0u;
    const uint32_t c = (uint32_t)__popcll(__ballot(occ));
    if (lane == 0) s_w[wave] = c;
    __syncthreads();
    if (tid == 0) {
        uint32_t r = 0;
        for (int w = 0; w < 16; w++) r += s_w[w];
        blk_rows[blockIdx.x] = r;
        if (r) atomicAdd(&meta[VS_META_ROWS], r);
    }
}

__global__ __launch_bounds__(kVsScanThreads) void vs_compact_kernel(VsTable T, uint64_t n_entries, const uint32_t* __restrict__ blk_rows, VsRows U,
                                                                    uint64_t row_base, uint32_t v0, uint32_t* meta)
{
    __shared__ unsigned long long s_w[16];
    __shared__ uint32_t s_mx;
    if (blk_rows[blockIdx.x] == 0) return;                   // (uniform: nine blocks in ten at the usual load)
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_mx = 0;
    unsigned long long pre = 0, before = 0;
    for (uint32_t b = tid; b < blockIdx.x; b += kVsScanThreads) pre += blk_rows[b];
    (void)vs_block_scan(pre, s_w, &before);                  // rows of all preceding blocks
    const uint64_t e = blockIdx.x * (uint64_t)kVsScanThreads + tid;
    const bool occ = e < n_entries && T.key[e] != 0u;
    unsigned long long tot = 0;
    const uint64_t row = row_base + before + vs_block_scan(occ ? 1ull : 0ull, s_w, &tot);
    uint32_t lab = 0;
    if (occ) {
        lab = T.key[e];
        U.vol[row] = v0 + (uint32_t)(e / T.cap); U.label[row] = lab; U.cnt[row] = T.cnt[e];
        U.x0[row] = T.xmin[e]; U.y0[row] = T.ymin[e]; U.z0[row] = T.zmin[e];
        U.w[row] = T.xmax[e] - T.xmin[e] + 1u; U.h[row] = T.ymax[e] - T.ymin[e] + 1u; U.d[row] = T.zmax[e] - T.zmin[e] + 1u;
        U.vmin[row] = T.vmin[e]; U.vmax[row] = T.vmax[e];
    }
    lab = vs_wave_max(lab);
    if (lane == 0 && lab) atomicMax(&s_mx, lab);
    __syncthreads();
    if (tid == 0) atomicMax(&meta[VS_META_MAX_LABEL], s_mx);
}

__global__ void vs_keys_kernel(VsRows U, uint64_t n, unsigned long long* keys, uint32_t* idx)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < n) { keys[i] = ((unsigned long long)U.vol[i] << 32) | U.label[i]; idx[i] = (uint32_t)i; }
}

// ---- the row sort ------------------------------------------------------------------------------------------------------------------
// hist[digit * n_blocks + block]: the exclusive prefix sum over this array in that order is where block `block` places its first key of
// digit `digit`.
__global__ __launch_bounds__(kVsSortThreads) void vs_sort_hist_kernel(const unsigned long long* __restrict__ keys, uint64_t n, int shift, uint32_t* hist)
{
    __shared__ uint32_t s_h[256];
    const int tid = threadIdx.x;
    s_h[tid] = 0;
    __syncthreads();
    const uint64_t t0 = blockIdx.x * (uint64_t)kVsSortTile;
#pragma unroll
    for (int r = 0; r < kVsSortRounds; r++) {
        const uint64_t i = t0 + (uint32_t)(r * kVsSortThreads + tid);
        if (i < n) atomicAdd(&s_h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(uint64_t)tid * gridDim.x + blockIdx.x] = s_h[tid];
}

// exclusive prefix sum of m words in place, one workgroup (m = 256 x blocks of the sort: a few thousand words for 10^5 rows)
__global__ __launch_bounds__(kVsScanThreads) void vs_scan_words_kernel(uint32_t* a, uint64_t m)
{
    __shared__ unsigned long long s_w[16];
    unsigned long long carry = 0;
    for (uint64_t i0 = 0; i0 < m; i0 += kVsScanThreads) {
        const uint64_t i = i0 + threadIdx.x;
        const unsigned long long v = i < m ? a[i] : 0u;
        unsigned long long tot = 0;
        const unsigned long long ex = vs_block_scan(v, s_w, &tot);
        if (i < m) a[i] = (uint32_t)(carry + ex);
        carry += tot;
    }
}

__global__ __launch_bounds__(kVsSortThreads) void vs_sort_scatter_kernel(const unsigned long long* __restrict__ keys_in, const uint32_t* __restrict__ idx_in,
                                                                         unsigned long long* keys_out, uint32_t* idx_out, uint64_t n, int shift,
                                                                         const uint32_t* __restrict__ hist)
{
    constexpr int NW = kVsSortThreads / 64;
    __shared__ uint32_t s_cnt[NW][256], s_run[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_run[tid] = hist[(uint64_t)tid * gridDim.x + blockIdx.x];
#pragma unroll
    for (int w = 0; w < NW; w++) s_cnt[w][tid] = 0;
    __syncthreads();
    const uint64_t t0 = blockIdx.x * (uint64_t)kVsSortTile;
    for (int r = 0; r < kVsSortRounds; r++) {
        const uint64_t i = t0 + (uint32_t)(r * kVsSortThreads + tid);
        const bool live = i < n;
        const unsigned long long key = live ? keys_in[i] : 0ull;
        const uint32_t d = (uint32_t)(key >> shift) & 255u;
        unsigned long long same = __ballot(live);            // the lanes of this step that hold my digit
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long bal = __ballot(live && one);
            same &= one ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (live && rank == 0) s_cnt[wave][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (live) {
            uint32_t pos = s_run[d] + rank;
            for (int w = 0; w < wave; w++) pos += s_cnt[w][d];
            keys_out[pos] = key; idx_out[pos] = idx_in[i];
        }
        __syncthreads();
        uint32_t adv = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) { adv += s_cnt[w][tid]; s_cnt[w][tid] = 0; }
        s_run[tid] += adv;
        __syncthreads();
    }
}

// ---- sorted rows, extrema, offsets ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vs_gather_kernel(VsRows U, const uint32_t* __restrict__ idx, uint64_t n, VsRows R, uint32_t* n_slab, uint32_t* meta)
{
    __shared__ uint32_t s_mx[3];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 3) s_mx[tid] = 0;
    __syncthreads();
    const uint64_t r = blockIdx.x * 256ull + tid;
    uint32_t m_px = 0, m_cells = 0, m_rng = 0;
    if (r < n) {
        const uint32_t s = idx[r];
        const uint32_t w = U.w[s], h = U.h[s], d = U.d[s], c = U.cnt[s], mn = U.vmin[s], mx = U.vmax[s];
        R.vol[r] = U.vol[s]; R.label[r] = U.label[s]; R.cnt[r] = c;
        R.x0[r] = U.x0[s]; R.y0[r] = U.y0[s]; R.z0[r] = U.z0[s]; R.w[r] = w; R.h[r] = h; R.d[r] = d; R.vmin[r] = mn; R.vmax[r] = mx;
        n_slab[r] = vs_slabs(w, h, d);
        const unsigned long long cells = (unsigned long long)w * h * d;   // (w * h * d < 2^32 * 2^16: no overflow)
        m_px = c; m_cells = cells > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cells; m_rng = mx - mn;
    }
    m_px = vs_wave_max(m_px); m_cells = vs_wave_max(m_cells); m_rng = vs_wave_max(m_rng);
    if (lane == 0) { atomicMax(&s_mx[0], m_px); atomicMax(&s_mx[1], m_cells); atomicMax(&s_mx[2], m_rng); }
    __syncthreads();
    if (tid == 0 && s_mx[0]) {
        atomicMax(&meta[VS_META_MAX_PX], s_mx[0]); atomicMax(&meta[VS_META_MAX_CELLS], s_mx[1]); atomicMax(&meta[VS_META_MAX_RANGE], s_mx[2]);
    }
}

// blk[2 b], blk[2 b + 1]: voxels and slabs of rows [1024 b, 1024 b + 1024)
__global__ __launch_bounds__(kVsScanThreads) void vs_offsets_sums_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ n_slab, uint64_t n,
                                                                         unsigned long long* blk)
{
    __shared__ unsigned long long s_w[16];
    const uint64_t r = blockIdx.x * (uint64_t)kVsScanThreads + threadIdx.x;
    unsigned long long ta = 0, tb = 0;
    (void)vs_block_scan(r < n ? cnt[r] : 0u, s_w, &ta);
    (void)vs_block_scan(r < n ? n_slab[r] : 0u, s_w, &tb);
    if (threadIdx.x == 0) { blk[2 * (uint64_t)blockIdx.x] = ta; blk[2 * (uint64_t)blockIdx.x + 1] = tb; }
}
// exclusive prefix sums over the nb pairs in place, one workgroup
__global__ __launch_bounds__(kVsScanThreads) void vs_offsets_scan_kernel(unsigned long long* blk, uint64_t nb)
{
    __shared__ unsigned long long s_w[16];
    unsigned long long ca = 0, cb = 0;
    for (uint64_t i0 = 0; i0 < nb; i0 += kVsScanThreads) {
        const uint64_t i = i0 + threadIdx.x;
        const unsigned long long a = i < nb ? blk[2 * i] : 0ull, b = i < nb ? blk[2 * i + 1] : 0ull;
        unsigned long long ta = 0, tb = 0;
        const unsigned long long ea = vs_block_scan(a, s_w, &ta), eb = vs_block_scan(b, s_w, &tb);
        if (i < nb) { blk[2 * i] = ca + ea; blk[2 * i + 1] = cb + eb; }
        ca += ta; cb += tb;
    }
}
__global__ __launch_bounds__(kVsScanThreads) void vs_offsets_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ n_slab, uint64_t n,
                                                                    const unsigned long long* __restrict__ blk, unsigned long long* px_offset,
                                                                    unsigned long long* slab_base)
{
    __shared__ unsigned long long s_w[16];
    const uint64_t r = blockIdx.x * (uint64_t)kVsScanThreads + threadIdx.x;
    const unsigned long long a = r < n ? cnt[r] : 0u, b = r < n ? n_slab[r] : 0u;
    unsigned long long ta = 0, tb = 0;
    const unsigned long long ea = blk[2 * (uint64_t)blockIdx.x] + vs_block_scan(a, s_w, &ta);
    const unsigned long long eb = blk[2 * (uint64_t)blockIdx.x + 1] + vs_block_scan(b, s_w, &tb);
    if (r < n) {
        px_offset[r] = ea; slab_base[r] = eb;
        if (r + 1 == n) { px_offset[n] = ea + a; slab_base[n] = eb + b; }   // the last row closes the offsets
    }
}

// One workgroup per (ROI, slab): see the head of the file.  COUNT: the hits of the slab -> slab_cnt (slabs of multi-slab boxes only).
template <typename TI, typename TL, bool COUNT>
__global__ __launch_bounds__(kVsCloudThreads) void vol_cloud_kernel(const TI* __restrict__ inten, const TL* __restrict__ label, uint32_t W, uint32_t H, uint32_t D,
                                                                    uint32_t v0, VsRows R, const unsigned long long* __restrict__ px_offset,
                                                                    const unsigned long long* __restrict__ slab_base, uint64_t r0, uint64_t r1, uint64_t slab0,
                                                                    uint32_t* slab_cnt, uint16_t* cx, uint16_t* cy, uint16_t* cz, uint32_t* cv)
{
    constexpr int U = kVsCloudUnroll, NW = kVsCloudThreads / 64;
    __shared__ uint32_t s_cnt[U * NW];
    __shared__ unsigned long long s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t slab = slab0 + blockIdx.x;
    uint64_t lo = r0, hi = r1;                               // slab_base[lo] <= slab < slab_base[hi]; every row has at least one slab
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (slab_base[mid] <= slab) lo = mid; else hi = mid;
    }
    const uint64_t row = lo;
    const uint64_t sb = slab_base[row];
    const uint32_t ns = (uint32_t)(slab_base[row + 1] - sb), s = (uint32_t)(slab - sb);
    if (COUNT && ns == 1) return;
    const uint32_t w = R.w[row], h = R.h[row], d = R.d[row], L = R.label[row];
    const uint32_t planes = vs_slab_planes(w, h, d);
    const uint32_t zs = s * planes, ze = zs + planes < d ? zs + planes : d;
    const uint32_t wh = w * h;                               // (w * h <= W * H < 2^32)
    const uint64_t cells = (uint64_t)wh * (ze - zs);
    const uint64_t base = (((uint64_t)(R.vol[row] - v0) * D + R.z0[row] + zs) * H + R.y0[row]) * W + R.x0[row];
    unsigned long long out = 0;
    if (!COUNT) {
        out = px_offset[row];
        if (s) {                                             // the prefix over the slabs in front of mine
            unsigned long long part = 0, tot = 0;
            for (uint32_t j = tid; j < s; j += kVsCloudThreads) part += slab_cnt[sb + j];
            (void)vs_block_scan(part, s_w, &tot);
            out += tot;
        }
    }
    uint32_t hits = 0;
    for (uint64_t p0 = 0; p0 < cells; p0 += kVsCloudThreads * U) {
        uint32_t lb[U], v[U], xs[U], ys[U], zz[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t p = p0 + (uint32_t)(u * kVsCloudThreads + tid);
            const bool ok = p < cells;
            const uint32_t q = ok ? (uint32_t)p : 0u;        // (cells < 2^32: a slab is one plane or at most kVsSlabCells cells)
            const uint32_t bz = q / wh, rem = q - bz * wh, by = rem / w, bx = rem - by * w;
            const uint64_t g = base + ((uint64_t)bz * H + by) * W + bx;
            xs[u] = bx; ys[u] = by; zz[u] = zs + bz;
            lb[u] = ok ? (uint32_t)label[g] : 0u;            // 0 is never a ROI label
            v[u] = 0;
            if (!COUNT) v[u] = ok ? (uint32_t)inten[g] : 0u;
        }
        unsigned long long bal[U];
        bool hit[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            hit[u] = lb[u] == L;
            bal[u] = __ballot(hit[u]);
            if (lane == 0) s_cnt[u * NW + wave] = (uint32_t)__popcll(bal[u]);
        }
        __syncthreads();
        uint32_t run = 0;                                    // hits of this trip before the current (piece, wave), in window order
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int w2 = 0; w2 < NW; w2++) {
                if (!COUNT && w2 == wave && hit[u]) {
                    const unsigned long long o = out + run + (uint32_t)__popcll(bal[u] & ((1ull << lane) - 1ull));
                    cx[o] = (uint16_t)xs[u]; cy[o] = (uint16_t)ys[u]; cz[o] = (uint16_t)zz[u]; cv[o] = v[u];
                }
                run += s_cnt[u * NW + w2];
            }
        }
        out += run; hits += run;
        __syncthreads();
    }
    if (COUNT && tid == 0) slab_cnt[slab] = hits;
}

// element-type dispatch: dt = 1 / 2 / 4 bytes per element
template <typename F>
int with_types(int dt_inten, int dt_label, F&& f)
{
#define NYX_TL(TI)                                                                  \
    switch (dt_label) {                                                             \
    case 1: return f((const TI*)nullptr, (const uint8_t*)nullptr);                  \
    case 2: return f((const TI*)nullptr, (const uint16_t*)nullptr);                 \
    case 4: return f((const TI*)nullptr, (const uint32_t*)nullptr);                 \
    default: return (int)hipErrorInvalidValue;                                      \
    }
    switch (dt_inten) {
    case 1: NYX_TL(uint8_t)
    case 2: NYX_TL(uint16_t)
    case 4: NYX_TL(uint32_t)
    default: return (int)hipErrorInvalidValue;
    }
#undef NYX_TL
}

inline unsigned blocks_of(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

} // namespace

int launch_vs_scan(const VsVolumes& V, VsTable T, uint32_t* meta, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint64_t n = (uint64_t)T.cap * V.n;
    hipLaunchKernelGGL(vs_init_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, T, n);
    const uint64_t planes = (uint64_t)V.D * V.n;             // (< 2^32: the host bounds the voxels of a chunk)
    const dim3 grid((V.W + kVsScanCols - 1) / kVsScanCols, (V.H + kVsScanRows - 1) / kVsScanRows,
                    (unsigned)(planes < (uint64_t)kVsMaxPlanesGrid ? planes : (uint64_t)kVsMaxPlanesGrid));
    const int rc = with_types(V.dt_inten, V.dt_label, [&](auto* ti, auto* tl) -> int {
        using TI = std::remove_const_t<std::remove_pointer_t<decltype(ti)>>;
        using TL = std::remove_const_t<std::remove_pointer_t<decltype(tl)>>;
        hipLaunchKernelGGL((vol_scan_kernel<TI, TL>), grid, dim3(kVsScanCols), 0, st, (const TI*)V.inten, (const TL*)V.label, V.W, V.H, V.D, (uint32_t)planes, T,
                           meta);
        return 0;
    });
    return rc ? rc : (int)hipGetLastError();
}

int launch_vs_count(VsTable T, uint64_t n_entries, uint32_t* blk_rows, uint32_t* meta, void* stream)
{
    hipLaunchKernelGGL(vs_count_kernel, dim3(blocks_of(n_entries, kVsScanThreads)), dim3(kVsScanThreads), 0, (hipStream_t)stream, T, n_entries, blk_rows, meta);
    return (int)hipGetLastError();
}

int launch_vs_compact(VsTable T, uint64_t n_entries, const uint32_t* blk_rows, VsRows U, uint64_t row_base, uint32_t v0, uint32_t* meta, void* stream)
{
    hipLaunchKernelGGL(vs_compact_kernel, dim3(blocks_of(n_entries, kVsScanThreads)), dim3(kVsScanThreads), 0, (hipStream_t)stream, T, n_entries, blk_rows, U,
                       row_base, v0, meta);
    return (int)hipGetLastError();
}

int launch_vs_keys(VsRows U, uint64_t n, unsigned long long* keys, uint32_t* idx, void* stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(vs_keys_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, (hipStream_t)stream, U, n, keys, idx);
    return (int)hipGetLastError();
}

int launch_vs_sort_pass(const unsigned long long* keys_in, const uint32_t* idx_in, unsigned long long* keys_out, uint32_t* idx_out, uint64_t n, int shift,
                        uint32_t* hist, void* stream)
{
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nb = vs_sort_blocks(n);
    hipLaunchKernelGGL(vs_sort_hist_kernel, dim3(nb), dim3(kVsSortThreads), 0, st, keys_in, n, shift, hist);
    hipLaunchKernelGGL(vs_scan_words_kernel, dim3(1), dim3(kVsScanThreads), 0, st, hist, 256ull * nb);
    hipLaunchKernelGGL(vs_sort_scatter_kernel, dim3(nb), dim3(kVsSortThreads), 0, st, keys_in, idx_in, keys_out, idx_out, n, shift, hist);
    return (int)hipGetLastError();
}

int launch_vs_gather(VsRows U, const uint32_t* idx, uint64_t n, VsRows R, uint32_t* n_slab, uint32_t* meta, void* stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(vs_gather_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, (hipStream_t)stream, U, idx, n, R, n_slab, meta);
    return (int)hipGetLastError();
}

int launch_vs_offsets(const uint32_t* cnt, const uint32_t* n_slab, uint64_t n, unsigned long long* blk_sums, unsigned long long* px_offset,
                      unsigned long long* slab_base, void* stream)
{
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = blocks_of(n, kVsScanThreads);
    hipLaunchKernelGGL(vs_offsets_sums_kernel, dim3(nb), dim3(kVsScanThreads), 0, st, cnt, n_slab, n, blk_sums);
    hipLaunchKernelGGL(vs_offsets_scan_kernel, dim3(1), dim3(kVsScanThreads), 0, st, blk_sums, (uint64_t)nb);
    hipLaunchKernelGGL(vs_offsets_kernel, dim3(nb), dim3(kVsScanThreads), 0, st, cnt, n_slab, n, blk_sums, px_offset, slab_base);
    return (int)hipGetLastError();
}

int launch_vs_clouds(const VsVolumes& V, VsRows R, const unsigned long long* px_offset, const unsigned long long* slab_base, uint64_t r0, uint64_t r1,
                     uint64_t slab0, uint64_t slab1, bool counted, uint32_t* slab_cnt, uint16_t* cx, uint16_t* cy, uint16_t* cz, uint32_t* cv, void* stream)
{
    if (slab1 <= slab0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(slab1 - slab0));
    const int rc = with_types(V.dt_inten, V.dt_label, [&](auto* ti, auto* tl) -> int {
        using TI = std::remove_const_t<std::remove_pointer_t<decltype(ti)>>;
        using TL = std::remove_const_t<std::remove_pointer_t<decltype(tl)>>;
        if (counted)
            hipLaunchKernelGGL((vol_cloud_kernel<TI, TL, true>), grid, dim3(kVsCloudThreads), 0, st, (const TI*)V.inten, (const TL*)V.label, V.W, V.H, V.D, V.v0, R,
                               px_offset, slab_base, r0, r1, slab0, slab_cnt, cx, cy, cz, cv);
        hipLaunchKernelGGL((vol_cloud_kernel<TI, TL, false>), grid, dim3(kVsCloudThreads), 0, st, (const TI*)V.inten, (const TL*)V.label, V.W, V.H, V.D, V.v0, R,
                           px_offset, slab_base, r0, r1, slab0, slab_cnt, cx, cy, cz, cv);
        return 0;
    });
    return rc ? rc : (int)hipGetLastError();
}

} // namespace nyxhip
