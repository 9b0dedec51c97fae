// The arithmetic of the device label scan for volumes (nyxus_amd/csrc/volscan_plan.h) on the host alone (no HIP, no library): the sizes
// of the per-volume label tables and how they grow, the probes of an insertion, the volumes of a chunk under a budget, the z-slabs of a
// box in the cloud launch and the passes of the row sort, held to literal numbers.  Prints one line per check and "ALL PASSED"; exit
// code 1 on a failure.
#include <cstdint>
#include <cstdio>

#include "../../nyxus_amd/csrc/volscan_plan.h"

using namespace nyxhip;

static int g_bad = 0;

static void expect(const char* what, uint64_t got, uint64_t want)
{
    const bool ok = got == want;
    printf("%s %s: %llu (want %llu)\n", ok ? "ok  " : "FAIL", what, (unsigned long long)got, (unsigned long long)want);
    if (!ok) g_bad++;
}

int main()
{
    // the constants the kernels and the tests' seams rest on
    expect("kVsScanCols", kVsScanCols, 256);
    expect("kVsScanRows", kVsScanRows, 32);
    expect("LDS table bytes", 8ull * 4 * kVsLdsCap, 16384);
    expect("kVsSortTile", kVsSortTile, 1024);

    expect("pow2ceil(0)", vs_pow2ceil(0), 1);
    expect("pow2ceil(1)", vs_pow2ceil(1), 1);
    expect("pow2ceil(3)", vs_pow2ceil(3), 4);
    expect("pow2ceil(4096)", vs_pow2ceil(4096), 4096);
    expect("pow2ceil(2^32 + 1)", vs_pow2ceil((1ull << 32) + 1), 1ull << 33);

    // table limits: twice the voxels, within [64, 2^24]
    expect("cap_limit(1 voxel)", vs_cap_limit(1), 64);
    expect("cap_limit(8000 voxels)", vs_cap_limit(8000), 16384);
    expect("cap_limit(128^3)", vs_cap_limit(128ull * 128 * 128), 1u << 22);
    expect("cap_limit(2^32 - 1 voxels)", vs_cap_limit(0xFFFFFFFFull), 1u << 24);
    expect("cap_first(limit 64, no hint)", vs_cap_first(64, 0), 64);
    expect("cap_first(limit 2^22, no hint)", vs_cap_first(1u << 22, 0), 4096);
    expect("cap_first(limit 2^22, hint 65536)", vs_cap_first(1u << 22, 65536), 65536);
    expect("cap_first(limit 16384, hint 2^22)", vs_cap_first(16384, 1u << 22), 16384);
    expect("cap_first(limit 2^22, hint 8)", vs_cap_first(1u << 22, 8), 64);

    // growth: times four up to the limit, 0 at the limit
    expect("cap_next(4096, 16384)", vs_cap_next(4096, 16384), 16384);
    expect("cap_next(4096, 8192)", vs_cap_next(4096, 8192), 8192);
    expect("cap_next(16384, 16384)", vs_cap_next(16384, 16384), 0);
    expect("cap_next(2^23, 2^24)", vs_cap_next(1u << 23, 1u << 24), 1u << 24);
    expect("cap_next(2^24, 2^24)", vs_cap_next(1u << 24, 1u << 24), 0);
    {   // the chain from the first table ends at the limit in a bounded number of scans
        uint32_t cap = vs_cap_first(1u << 24, 0), scans = 1;
        while (uint32_t n = vs_cap_next(cap, 1u << 24)) { cap = n; scans++; }
        expect("scans from 4096 to 2^24", scans, 7);
        expect("last table", cap, 1u << 24);
    }
    expect("probes(4096, limit 2^22)", vs_probes(4096, 1u << 22), 1024);
    expect("probes(64, limit 2^22)", vs_probes(64, 1u << 22), 64);
    expect("probes(16384 at its limit)", vs_probes(16384, 16384), 16384);
    expect("log2(4096)", vs_log2(4096), 12);

    expect("table_bytes(4096)", vs_table_bytes(4096), 163840);
    expect("volume_bytes(1000 voxels, u16, u8)", vs_volume_bytes(1000, 2, 1), 2048 + 1024);
    expect("volume_bytes(2^32 - 1 voxels, u32, u32)", vs_volume_bytes(0xFFFFFFFFull, 4, 4), 2 * ((4 * 0xFFFFFFFFull + 255) & ~255ull));

    // chunks
    expect("chunk: budget of 2.5 volumes", vs_chunk_volumes(2 * (3072 + 163840) + 90000, 3072, 4096, 3), 2);
    expect("chunk: all fit", vs_chunk_volumes(1ull << 30, 3072, 4096, 3), 3);
    expect("chunk: one byte short of a volume", vs_chunk_volumes(3072 + 163840 - 1, 3072, 4096, 3), 0);
    expect("chunk: device volumes stage nothing", vs_chunk_volumes(163840, 0, 4096, 3), 1);

    // slabs of the cloud launch
    expect("slab_planes(32 x 32 x 32)", vs_slab_planes(32, 32, 32), 32);
    expect("slabs(32 x 32 x 32)", vs_slabs(32, 32, 32), 1);
    expect("slab_planes(32 x 32 x 33)", vs_slab_planes(32, 32, 33), 32);
    expect("slabs(32 x 32 x 33)", vs_slabs(32, 32, 33), 2);
    expect("slab_planes(256^3)", vs_slab_planes(256, 256, 256), 1);
    expect("slabs(256^3)", vs_slabs(256, 256, 256), 256);
    expect("slab_planes(65534 x 65534 plane)", vs_slab_planes(65534, 65534, 1), 1);
    expect("slabs(1000 x 1000 x 1)", vs_slabs(1000, 1000, 1), 1);
    expect("slabs(1 x 1 x 65534)", vs_slabs(1, 1, 65534), 2);
    expect("slabs(1 x 1 x 1)", vs_slabs(1, 1, 1), 1);
    {   // the slabs of a box cover its planes exactly once
        const uint32_t w = 33, h = 31, d = 77, p = vs_slab_planes(w, h, d), n = vs_slabs(w, h, d);
        expect("cover: last slab begins inside", (uint64_t)(n - 1) * p < d, 1);
        expect("cover: slabs reach the end", (uint64_t)n * p >= d, 1);
        expect("cover: a slab holds at most kVsSlabCells", (uint64_t)w * h * p <= kVsSlabCells, 1);
    }

    // sort passes
    expect("label_passes(1)", vs_label_passes(1), 1);
    expect("label_passes(255)", vs_label_passes(255), 1);
    expect("label_passes(256)", vs_label_passes(256), 2);
    expect("label_passes(100000)", vs_label_passes(100000), 3);
    expect("label_passes(2^32 - 1)", vs_label_passes(0xFFFFFFFFu), 4);
    expect("volume_passes(1)", vs_volume_passes(1), 0);
    expect("volume_passes(2)", vs_volume_passes(2), 1);
    expect("volume_passes(256)", vs_volume_passes(256), 1);
    expect("volume_passes(257)", vs_volume_passes(257), 2);
    expect("volume_passes(2^32 - 1)", vs_volume_passes(0xFFFFFFFFu), 4);
    expect("sort_blocks(1)", vs_sort_blocks(1), 1);
    expect("sort_blocks(1024)", vs_sort_blocks(1024), 1);
    expect("sort_blocks(1025)", vs_sort_blocks(1025), 2);
    expect("sort_blocks(2^31 - 1)", vs_sort_blocks(0x7FFFFFFFull), 1u << 21);

    if (g_bad) printf("%d FAILED\n", g_bad);
    else printf("ALL PASSED\n");
    return g_bad ? 1 : 0;
}
