// volscan_plan.h -- the arithmetic of the device label scan for volumes (nyxhip_assemble_volumes), in plain C++ (no HIP:
// tests/cpp/test_volscan_plan.cpp includes it with g++): the constants of vol_assembly.hip, the sizes of the per-volume label tables and
// how they grow, the volumes of a chunk under the budget, the z-slabs of a box in the cloud launch, the passes of the row sort, and the
// argument blocks of the launches.  nyxhip_volscan.hip carves its workspaces by these numbers; vol_assembly.hip has the kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NYX_VS_HD __host__ __device__
#else
#define NYX_VS_HD
#endif

namespace nyxhip {

// ---- the scan block: kVsScanCols columns x kVsScanRows rows of ONE z-plane per workgroup, one thread per column -------------------
constexpr int kVsScanCols = 256;
constexpr int kVsScanRows = 32;
constexpr int kVsScanBatch = 8;          // loads of a column in flight
constexpr int kVsLdsCap = 512;           // slots of the workgroup's LDS label table (8 words each: 16 KiB)
constexpr int kVsLdsProbes = 32;         // probes before a run goes straight to the volume's table in HBM
constexpr int kVsMaxPlanesGrid = 65535;  // grid.z; the workgroups stride over the z-planes beyond it

// ---- the per-volume open-addressing table in HBM: kVsTableWords arrays of `cap` words (key, count, vmin, vmax, min / max of x, y, z) --
constexpr int kVsTableWords = 10;
constexpr uint32_t kVsCapMin = 64;
constexpr uint32_t kVsCapFirst = 4096;   // the first table of a context; later calls start at the size that served the last one
constexpr uint32_t kVsCapGrow = 4;       // a table that overflows is replaced by one this many times larger, and the chunk is scanned again
constexpr uint32_t kVsCapMax = 1u << 24; // the stated maximum: a volume with more labels than this is refused
constexpr uint32_t kVsProbeCap = 1024;   // probes of a table below its limit (a table AT its limit is probed all around)

// ---- the cloud launch: a box of more than kVsSlabCells cells is cut into slabs of whole z-planes, a workgroup each --------------------
constexpr uint32_t kVsSlabCells = 1u << 15;
constexpr int kVsCloudThreads = 256;
constexpr int kVsCloudUnroll = 4;        // 256-cell pieces of the window per trip

// ---- the row sort: LSD radix over (volume, label), 8 bits a pass, kVsSortTile keys per workgroup -------------------------------------
constexpr int kVsSortThreads = 256;
constexpr int kVsSortRounds = 4;
constexpr int kVsSortTile = kVsSortThreads * kVsSortRounds;
constexpr int kVsScanThreads = 1024;     // the prefix-sum and compaction launches

constexpr uint32_t kVsMaxSide = 65534;   // coordinates inside a box are 16-bit

// words of the device meta block
enum { VS_META_STATUS = 0,               // 1: a volume's table overflowed
       VS_META_ROWS = 1,                 // occupied slots of the chunk
       VS_META_MAX_LABEL = 2,
       VS_META_MAX_PX = 3, VS_META_MAX_CELLS = 4, VS_META_MAX_RANGE = 5,
       VS_META_WORDS = 16 };

NYX_VS_HD inline uint64_t vs_pow2ceil(uint64_t v)
{
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// The largest table a volume of `voxels` voxels can need: twice its voxels (it has at most `voxels` labels, so a table of that size is
// never more than half full), within [kVsCapMin, kVsCapMax].
inline uint32_t vs_cap_limit(uint64_t voxels)
{
    const uint64_t p = vs_pow2ceil(2 * voxels);
    return (uint32_t)(p < kVsCapMin ? kVsCapMin : p > kVsCapMax ? kVsCapMax : p);
}
// The table a call starts with: `hint` (the size that served the context's last call; 0: none) or kVsCapFirst, within the limit.
inline uint32_t vs_cap_first(uint32_t limit, uint32_t hint)
{
    uint32_t c = hint ? hint : kVsCapFirst;
    if (c < kVsCapMin) c = kVsCapMin;
    return c < limit ? c : limit;
}
// The table after an overflow of `cap`; 0: `cap` was the limit already (the volume holds more labels than the stated maximum).
inline uint32_t vs_cap_next(uint32_t cap, uint32_t limit)
{
    if (cap >= limit) return 0;
    const uint64_t n = (uint64_t)cap * kVsCapGrow;
    return (uint32_t)(n < limit ? n : limit);
}
// Probes of an insertion: all around a table at its limit (an overflow there is final), kVsProbeCap below it (a crowded table is
// replaced sooner than it is searched all around).
inline uint32_t vs_probes(uint32_t cap, uint32_t limit) { return cap >= limit || cap < kVsProbeCap ? cap : kVsProbeCap; }
inline uint32_t vs_log2(uint32_t pow2)
{
    uint32_t s = 0;
    while ((1u << s) < pow2) s++;
    return s;
}
inline size_t vs_al256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t vs_table_bytes(uint32_t cap) { return (size_t)kVsTableWords * 4 * cap; }
inline uint64_t vs_volume_bytes(uint64_t voxels, int dt_inten, int dt_label) { return vs_al256(voxels * (uint64_t)dt_inten) + vs_al256(voxels * (uint64_t)dt_label); }

// Volumes per chunk: as many of the `left` volumes as fit the budget with their tables (and, for host volumes, their staged bytes);
// 0: one volume does not fit.
inline uint32_t vs_chunk_volumes(uint64_t budget, uint64_t staged_bytes_per_volume, uint32_t cap, uint32_t left)
{
    const uint64_t per = staged_bytes_per_volume + vs_table_bytes(cap);
    const uint64_t fit = budget / per;
    return (uint32_t)(fit < left ? fit : left);
}

// z-planes per slab of a w x h x d box and its slabs: one slab while the box has at most kVsSlabCells cells, else slabs of as many
// whole planes as hold at most kVsSlabCells cells (at least one plane).
NYX_VS_HD inline uint32_t vs_slab_planes(uint32_t w, uint32_t h, uint32_t d)
{
    const uint64_t plane = (uint64_t)w * h;
    if (plane * d <= kVsSlabCells) return d;
    const uint64_t p = kVsSlabCells / plane;
    return p ? (uint32_t)p : 1u;
}
NYX_VS_HD inline uint32_t vs_slabs(uint32_t w, uint32_t h, uint32_t d)
{
    const uint32_t p = vs_slab_planes(w, h, d);
    return (d + p - 1) / p;
}

// Passes of the row sort (8 bits each): the bytes of the largest label, then the bytes of the largest volume index.  Cost of the sort:
// passes x (one read of the keys for the digit counts + one read and one write for the stable scatter): linear in the rows.
inline int vs_label_passes(uint32_t max_label)
{
    int p = 1;
    while (p < 4 && (max_label >> (8 * p)) != 0) p++;
    return p;
}
inline int vs_volume_passes(uint32_t n_volumes)
{
    int p = 0;
    while (p < 4 && ((uint64_t)(n_volumes - 1) >> (8 * p)) != 0) p++;
    return p;
}
inline uint32_t vs_sort_blocks(uint64_t n) { return (uint32_t)((n + kVsSortTile - 1) / kVsSortTile); }

// ---- argument blocks of the launches (device pointers) ---------------------------------------------------------------------------
struct VsTable {             // the tables of a chunk's volumes, each array [n_volumes_of_chunk * cap]; key 0 = empty slot
    uint32_t *key, *cnt, *vmin, *vmax, *xmin, *xmax, *ymin, *ymax, *zmin, *zmax;
    uint32_t cap, probes;
};
struct VsRows {              // one entry per ROI; `vol` is the index into the caller's stack
    uint32_t *vol, *label, *cnt, *x0, *y0, *z0, *w, *h, *d, *vmin, *vmax;
};
constexpr int kVsRowWords = 11;
struct VsVolumes {           // the volumes of a chunk in device memory
    const void* inten;
    const void* label;
    int dt_inten, dt_label;
    uint32_t W, H, D, n, v0; // n volumes, the first of which is volume v0 of the stack
};

// vol_assembly.hip: every launch is enqueued on `stream`; the return value is a hipError_t
int launch_vs_scan(const VsVolumes& V, VsTable T, uint32_t* meta, void* stream);                               // clears the tables, then scans
int launch_vs_count(VsTable T, uint64_t n_entries, uint32_t* blk_rows, uint32_t* meta, void* stream);          // occupied slots per 1024 entries, their sum in meta
int launch_vs_compact(VsTable T, uint64_t n_entries, const uint32_t* blk_rows, VsRows U, uint64_t row_base, uint32_t v0, uint32_t* meta, void* stream);
int launch_vs_keys(VsRows U, uint64_t n, unsigned long long* keys, uint32_t* idx, void* stream);
// one pass of the sort: digit `shift` of keys_in -> keys_out / idx_out; hist: [256 * vs_sort_blocks(n)] words
int launch_vs_sort_pass(const unsigned long long* keys_in, const uint32_t* idx_in, unsigned long long* keys_out, uint32_t* idx_out, uint64_t n, int shift,
                        uint32_t* hist, void* stream);
// sorted rows R[r] = U[idx[r]], the slabs of every row, the three extrema into meta; then px_offset [n + 1] and slab_base [n + 1]
int launch_vs_gather(VsRows U, const uint32_t* idx, uint64_t n, VsRows R, uint32_t* n_slab, uint32_t* meta, void* stream);
int launch_vs_offsets(const uint32_t* cnt, const uint32_t* n_slab, uint64_t n, unsigned long long* blk_sums /* [2 * ceil(n / 1024)] */,
                      unsigned long long* px_offset, unsigned long long* slab_base, void* stream);
// the clouds of rows [r0, r1) (all of volumes of V), whose slabs are [slab0, slab1): the count pass when `counted`, then the write pass
int launch_vs_clouds(const VsVolumes& V, VsRows R, const unsigned long long* px_offset, const unsigned long long* slab_base, uint64_t r0, uint64_t r1,
                     uint64_t slab0, uint64_t slab1, bool counted, uint32_t* slab_cnt, uint16_t* cx, uint16_t* cy, uint16_t* cz, uint32_t* cv, void* stream);

} // namespace nyxhip
