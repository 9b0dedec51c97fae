// vol_chunk, vol_sides and the *_layout functions of nyxus_amd/csrc/vol_plan.h: the arithmetic of the volume entries' workspaces, on the
// host alone (no HIP, no library; the device qualifiers of the kernel headers are defined away).  The expected strides and bytes per
// ROI are literals, worked out from the expressions the four entries carried before they shared this header.  Prints one line per
// check and "ALL PASSED"; exit code 1 on a failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#define __host__
#define __device__
#include "../../nyxus_amd/csrc/vol_plan.h"

using namespace nyxhip;

// shifts13[] of the reference's 3d_glrlm.cpp:17-32 as (dz, dy, dx): the library has them in its zone kernel unit
const int nyxhip::kVzShifts[kVzDirs][3] = {{1, 1, 1}, {1, 1, 0}, {1, 1, -1}, {1, 0, 1}, {1, 0, 0}, {1, 0, -1}, {1, -1, 1},
                                           {1, -1, 0}, {1, -1, -1}, {0, 1, 1}, {0, 1, 0}, {0, 1, -1}, {0, 0, 1}};

static int g_bad = 0;

static void expect(const char* what, uint64_t got, uint64_t want)
{
    const bool ok = got == want;
    printf("%s %s: %llu (want %llu)\n", ok ? "ok  " : "FAIL", what, (unsigned long long)got, (unsigned long long)want);
    if (!ok) g_bad++;
}

static void expect_all(const char* family, const char* what, unsigned long long mc, const std::vector<uint64_t>& got, const std::vector<uint64_t>& want)
{
    const bool ok = got == want;
    printf("%s %s, %s, max_cells %llu:", ok ? "ok  " : "FAIL", family, what, mc);
    for (size_t i = 0; i < got.size(); i++) printf(" %llu", (unsigned long long)got[i]);
    if (!ok) {
        printf(" (want");
        for (size_t i = 0; i < want.size(); i++) printf(" %llu", (unsigned long long)want[i]);
        printf(")");
        g_bad++;
    }
    printf("\n");
}

static nyxhip_settings settings(int grey_depth)
{
    nyxhip_settings s = {};
    s.grey_depth = grey_depth;
    return s;
}

// box_stride, tab_stride[GLDM, NGLDM, NGTDM], the NGTDM sweep runs, GLDM and NGTDM share a box, per_roi
static void tex(const char* what, uint32_t mask, int g_gldm, int g_ngtdm, int radius, uint32_t max_cells, const std::vector<uint64_t>& want)
{
    const nyxhip_settings s = settings(64);
    const nyxhip_voltex_settings t = {g_gldm, g_ngtdm, radius};
    VoltexArgs a = {};
    const VoltexLayout L = voltex_layout(a, mask, &s, &t, max_cells);
    expect_all("textures", what, max_cells, {a.box_stride, a.tab_stride[VT_GLDM], a.tab_stride[VT_NGLDM], a.tab_stride[VT_NGTDM], L.tsweep, L.share, L.per_roi}, want);
    if (L.tab_words != a.tab_stride[0] + a.tab_stride[1] + a.tab_stride[2] || a.max_cells != max_cells) { printf("FAIL textures, %s: tab_words / max_cells\n", what); g_bad++; }
}

// box_stride, rl_stride, rl_dir_off[12], sz_stride, cell_stride, key_stride, the classes share a box, per_roi
static void zone(const char* what, uint32_t mask, int g_glrlm, int g_glszm, uint32_t max_cells, VolSides sides, const std::vector<uint64_t>& want)
{
    const nyxhip_settings s = settings(64);
    const nyxhip_volzone_settings t = {g_glrlm, g_glszm};
    VolzoneArgs a = {};
    const VolzoneLayout L = volzone_layout(a, mask, &s, &t, max_cells, sides);
    char name[128];
    snprintf(name, sizeof(name), "%s, sides %u x %u x %u", what, sides.side_max[0], sides.side_max[1], sides.side_max[2]);
    expect_all("zones", name, max_cells, {a.box_stride, a.rl_stride, a.rl_dir_off[12], a.sz_stride, a.cell_stride, a.key_stride, L.share, L.per_roi}, want);
    if (L.tab_words != a.rl_stride + a.sz_stride || a.side_max[0] != sides.side_max[0] || a.side_max[2] != sides.side_max[2]) { printf("FAIL zones, %s: tab_words / side_max\n", name); g_bad++; }
}

// rows, box_stride, tab_stride, cell_stride, dist_stride, per_roi
static void dzone(const char* what, int grey_depth, uint32_t max_cells, uint32_t pitch, const std::vector<uint64_t>& want)
{
    const nyxhip_settings s = settings(grey_depth);
    const VolSides sides = {{7, 5, 3}, pitch};
    VoldzoneArgs a = {};
    const size_t per_roi = voldzone_layout(a, &s, max_cells, sides);
    char name[128];
    snprintf(name, sizeof(name), "%s, pitch %u", what, pitch);
    expect_all("distance zones", name, max_cells, {a.rows, a.box_stride, a.tab_stride, a.cell_stride, a.dist_stride, per_roi}, want);
    if (a.pitch_max != pitch || a.side_max[1] != 5) { printf("FAIL distance zones, %s: pitch_max / side_max\n", name); g_bad++; }
}

// box_stride, key_stride, per_roi
static void volm(const char* what, uint32_t mask, uint32_t max_px, uint32_t max_cells, const std::vector<uint64_t>& want)
{
    const nyxhip_settings s = settings(64);
    VolArgs a = {};
    const size_t per_roi = vol_layout(a, mask, &s, max_px, max_cells);
    char name[128];
    snprintf(name, sizeof(name), "%s, max_px %u", what, max_px);
    expect_all("volumes", name, max_cells, {a.box_stride, a.key_stride, per_roi}, want);
}

static void fold(const char* what, const std::vector<uint32_t>& w, const std::vector<uint32_t>& h, const std::vector<uint32_t>& d, uint32_t max_cells,
                 const std::vector<uint64_t>& want)
{
    const VolSides m = vol_sides(w.size(), w.data(), h.data(), d.data(), max_cells);
    expect_all("sides", what, max_cells, {m.side_max[0], m.side_max[1], m.side_max[2], m.pitch_max}, want);
}

int main()
{
    // the ROIs of a chunk
    expect("a budget below per_roi does not fit", vol_chunk(100, 99, 10), 0);
    expect("a budget of per_roi", vol_chunk(100, 100, 10), 1);
    expect("a budget of 3 * per_roi + 5", vol_chunk(100, 305, 10), 3);
    expect("a budget for 100000 ROIs", vol_chunk(100, 10000000, 200000), 65535);
    expect("a batch of 1 ROI", vol_chunk(100, 10000000, 1), 1);
    expect("per_roi 0 is not divided by, 10 ROIs", vol_chunk(0, 0, 10), 10);
    expect("per_roi 0 is not divided by, 100000 ROIs", vol_chunk(0, 0, 100000), 65535);

    // the box sides of a batch
    fold("a side of 65535 is refused", {65535, 3}, {1, 2}, {1, 2}, 1u << 24, {3, 2, 2, 3});
    fold("a side of 65534 is admitted", {65534, 3}, {1, 2}, {1, 2}, 1u << 24, {65534, 2, 2, 3});
    fold("cells beyond max_cells raise no maximum", {11, 10}, {10, 10}, {10, 10}, 1000, {10, 10, 10, 7});
    fold("an all-refused batch", {65535, 11}, {1, 10}, {1, 10}, 1000, {1, 1, 1, 2});
    fold("an empty batch", {}, {}, {}, 1000, {1, 1, 1, 2});
    fold("w, h, d and min(w, h) from four ROIs", {9, 2, 2, 6}, {2, 8, 2, 6}, {2, 2, 7, 1}, 1000, {9, 8, 7, 5});

    // strides and bytes per ROI of each entry
    tex("ALL, radius 1, depths 16 / 32", 7, 16, 32, 1, 1u, {256ull, 3520ull, 3264ull, 2240ull, 1ull, 0ull, 36864ull});
    tex("ALL, radius 1, depths 16 / 16", 7, 16, 16, 1, 1u, {256ull, 3520ull, 3264ull, 2240ull, 1ull, 1ull, 36608ull});
    tex("NGTDM alone, radius 0", 4, 16, 32, 0, 1u, {256ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull});
    tex("ALL, radius 1, depths 16 / 32", 7, 16, 32, 1, 1000u, {1024ull, 3520ull, 3264ull, 2240ull, 1ull, 0ull, 39168ull});
    tex("ALL, radius 1, depths 16 / 16", 7, 16, 16, 1, 1000u, {1024ull, 3520ull, 3264ull, 2240ull, 1ull, 1ull, 38144ull});
    tex("NGTDM alone, radius 0", 4, 16, 32, 0, 1000u, {1024ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull});
    tex("ALL, radius 1, depths 16 / 32", 7, 16, 32, 1, 16777216u, {16777216ull, 3520ull, 3264ull, 2240ull, 1ull, 0ull, 50367744ull});
    tex("ALL, radius 1, depths 16 / 16", 7, 16, 16, 1, 16777216u, {16777216ull, 3520ull, 3264ull, 2240ull, 1ull, 1ull, 33590528ull});
    tex("NGTDM alone, radius 0", 4, 16, 32, 0, 16777216u, {16777216ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull});
    zone("ALL, depths 16 / 16", 3, 16, 16, 1u, {1, 1, 1}, {256ull, 256ull, 220ull, 576ull, 64ull, 64ull, 1ull, 4608ull});
    zone("ALL, depths 16 / 32", 3, 16, 32, 1u, {1, 1, 1}, {256ull, 256ull, 220ull, 1088ull, 64ull, 64ull, 0ull, 6912ull});
    zone("ALL, depths 16 / 16", 3, 16, 16, 1u, {7, 5, 3}, {256ull, 896ull, 730ull, 576ull, 64ull, 64ull, 1ull, 7168ull});
    zone("ALL, depths 16 / 32", 3, 16, 32, 1u, {7, 5, 3}, {256ull, 896ull, 730ull, 1088ull, 64ull, 64ull, 0ull, 9472ull});
    zone("GLRLM alone, depth 0", 1, 0, 0, 1u, {7, 5, 3}, {256ull, 6400ull, 5434ull, 0ull, 0ull, 0ull, 0ull, 25856ull});
    zone("GLSZM alone, depth -20", 2, 16, -20, 1u, {7, 5, 3}, {256ull, 0ull, 0ull, 704ull, 64ull, 64ull, 0ull, 4096ull});
    zone("ALL, depths 16 / 16", 3, 16, 16, 1000u, {1, 1, 1}, {1024ull, 256ull, 220ull, 576ull, 1024ull, 64ull, 1ull, 13056ull});
    zone("ALL, depths 16 / 32", 3, 16, 32, 1000u, {1, 1, 1}, {1024ull, 256ull, 220ull, 1088ull, 1024ull, 64ull, 0ull, 16128ull});
    zone("ALL, depths 16 / 16", 3, 16, 16, 1000u, {7, 5, 3}, {1024ull, 896ull, 730ull, 576ull, 1024ull, 64ull, 1ull, 15616ull});
    zone("ALL, depths 16 / 32", 3, 16, 32, 1000u, {7, 5, 3}, {1024ull, 896ull, 730ull, 1088ull, 1024ull, 64ull, 0ull, 18688ull});
    zone("GLRLM alone, depth 0", 1, 0, 0, 1000u, {7, 5, 3}, {1024ull, 6400ull, 5434ull, 0ull, 0ull, 0ull, 0ull, 26624ull});
    zone("GLSZM alone, depth -20", 2, 16, -20, 1000u, {7, 5, 3}, {1024ull, 0ull, 0ull, 704ull, 1024ull, 64ull, 0ull, 12544ull});
    zone("ALL, depths 16 / 16", 3, 16, 16, 16777216u, {1, 1, 1}, {16777216ull, 256ull, 220ull, 576ull, 16777216ull, 508416ull, 1ull, 155065600ull});
    zone("ALL, depths 16 / 32", 3, 16, 32, 16777216u, {1, 1, 1}, {16777216ull, 256ull, 220ull, 1088ull, 16777216ull, 508416ull, 0ull, 171844864ull});
    zone("ALL, depths 16 / 16", 3, 16, 16, 16777216u, {7, 5, 3}, {16777216ull, 896ull, 730ull, 576ull, 16777216ull, 508416ull, 1ull, 155068160ull});
    zone("ALL, depths 16 / 32", 3, 16, 32, 16777216u, {7, 5, 3}, {16777216ull, 896ull, 730ull, 1088ull, 16777216ull, 508416ull, 0ull, 171847424ull});
    zone("GLRLM alone, depth 0", 1, 0, 0, 16777216u, {7, 5, 3}, {16777216ull, 6400ull, 5434ull, 0ull, 0ull, 0ull, 0ull, 16802816ull});
    zone("GLSZM alone, depth -20", 2, 16, -20, 16777216u, {7, 5, 3}, {16777216ull, 0ull, 0ull, 704ull, 16777216ull, 508416ull, 0ull, 155065088ull});
    dzone("grey depth 0", 0, 1u, 2u, {129ull, 256ull, 320ull, 64ull, 128ull, 2304ull});
    dzone("grey depth 0", 0, 1u, 4u, {129ull, 256ull, 576ull, 64ull, 128ull, 3328ull});
    dzone("grey depth 16", 16, 1u, 2u, {17ull, 256ull, 64ull, 64ull, 128ull, 1280ull});
    dzone("grey depth 16", 16, 1u, 4u, {17ull, 256ull, 128ull, 64ull, 128ull, 1536ull});
    dzone("grey depth 0", 0, 1000u, 2u, {129ull, 1024ull, 320ull, 1024ull, 1024ull, 12544ull});
    dzone("grey depth 0", 0, 1000u, 4u, {129ull, 1024ull, 576ull, 1024ull, 1024ull, 13568ull});
    dzone("grey depth 16", 16, 1000u, 2u, {17ull, 1024ull, 64ull, 1024ull, 1024ull, 11520ull});
    dzone("grey depth 16", 16, 1000u, 4u, {17ull, 1024ull, 128ull, 1024ull, 1024ull, 11776ull});
    dzone("grey depth 0", 0, 16777216u, 2u, {129ull, 16777216ull, 320ull, 16777216ull, 16777216ull, 184550656ull});
    dzone("grey depth 0", 0, 16777216u, 4u, {129ull, 16777216ull, 576ull, 16777216ull, 16777216ull, 184551680ull});
    dzone("grey depth 16", 16, 16777216u, 2u, {17ull, 16777216ull, 64ull, 16777216ull, 16777216ull, 184549632ull});
    dzone("grey depth 16", 16, 16777216u, 4u, {17ull, 16777216ull, 128ull, 16777216ull, 16777216ull, 184549888ull});
    volm("intensity alone", 1, 1u, 1u, {0ull, 64ull, 512ull});
    volm("intensity alone", 1, 999u, 1u, {0ull, 1024ull, 8192ull});
    volm("GLCM alone", 2, 1u, 1u, {256ull, 0ull, 256ull});
    volm("GLCM alone", 2, 999u, 1u, {256ull, 0ull, 256ull});
    volm("both", 3, 1u, 1u, {256ull, 64ull, 768ull});
    volm("both", 3, 999u, 1u, {256ull, 1024ull, 8448ull});
    volm("intensity alone", 1, 999u, 1000u, {0ull, 1024ull, 8192ull});
    volm("GLCM alone", 2, 999u, 1000u, {1024ull, 0ull, 1024ull});
    volm("both", 3, 999u, 1000u, {1024ull, 1024ull, 9216ull});
    volm("intensity alone", 1, 999u, 16777216u, {0ull, 1024ull, 8192ull});
    volm("intensity alone", 1, 5000000u, 16777216u, {0ull, 5000000ull, 40000000ull});
    volm("GLCM alone", 2, 999u, 16777216u, {16777216ull, 0ull, 16777216ull});
    volm("GLCM alone", 2, 5000000u, 16777216u, {16777216ull, 0ull, 16777216ull});
    volm("both", 3, 999u, 16777216u, {16777216ull, 1024ull, 16785408ull});
    volm("both", 3, 5000000u, 16777216u, {16777216ull, 5000000ull, 56777216ull});
    // the settings and extrema of the mixed batches of tests/test_vol*_gpu.py (test_a_row_has_the_same_bits_however_it_is_asked_for): the
    // last number of each is the N of the library's "workspace of one ROI (N bytes) does not fit" refusal on those batches
    volm("the mixed batch", 3, 38240u, 64000u, {64000ull, 38272ull, 370176ull});
    tex("the mixed batch: ALL, radius 2, depths -20 / 16", 7, -20, 16, 2, 65538u, {65792ull, 3520ull, 3264ull, 7104ull, 1ull, 0ull, 252928ull});
    zone("the mixed batch: ALL, depths -8 / 6", 3, -8, 6, 47952u, {{8191, 68, 68}, 20}, {48128ull, 81088ull, 7360ull, 256ull, 48000ull, 1472ull, 0ull, 817408ull});
    {
        const nyxhip_settings s = settings(0);
        VoldzoneArgs a = {};
        const VolSides sides = {{241, 17, 13}, 10};
        expect("distance zones, the mixed batch: per_roi", voldzone_layout(a, &s, 8194, sides), 96512);
        expect("distance zones, the mixed batch: tab_stride", a.tab_stride, 1344);
    }
    // stated extrema of 0 count as 1; IBSI mode ignores the grey depths (the distance zones take all 129 rows)
    volm("both, max_cells 0", 3, 0, 0, {256ull, 64ull, 768ull});
    {
        nyxhip_settings s = settings(16);
        s.ibsi = 1;
        VoldzoneArgs a = {};
        const VolSides sides = {{1, 1, 1}, 2};
        expect("distance zones, IBSI: per_roi", voldzone_layout(a, &s, 1, sides), 2304);
        expect("distance zones, IBSI: rows", a.rows, 129);
    }
    if (g_bad) { printf("%d FAILED\n", g_bad); return 1; }
    printf("ALL PASSED\n");
    return 0;
}
