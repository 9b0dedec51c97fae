// features_plan.h -- the builds of the metric kernel (roi_features.hip) and the rule that picks one, in plain C++ (no HIP header, no
// look at the environment: tests/cpp/test_features_plan.cpp includes it with g++, the device qualifiers of roi_kernel.h defined away).
//   NYX_FEATURE_BUILDS     every build of roi_features_kernel, once, as a row of template arguments.  roi_features.hip expands it
//                          into the kernel pointers (which instantiates them); the per-device opt-in and the lookup walk both tables.
//   plan_features_launch   what launch_roi_features does for a set of arguments: the engine (roi_small, or a build of the table), its
//                          geometry, and the launches that follow it.  A function of its arguments alone.
//   lds_workgroups_per_cu  the occupancy rule of the LDS launches (the tiers of the plan, make_layout's first-moment prefixes).
//   glcm_wave_lds / glcm8_wave_lds   per-wave carve-outs of the two GLCM feature kernels, for the kernels and their launches.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "roi_kernel.h"

namespace nyxhip {

constexpr size_t kLdsPerCu = 160 * 1024;   // gfx950: 160 KiB per CU, all of it usable by one workgroup (roi_features_max_lds)

// workgroups of `total` bytes of LDS that share a CU: eight at the most (64-VGPR builds of four waves)
__host__ __device__ inline uint32_t lds_workgroups_per_cu(uint32_t total)
{
    const uint32_t n = (uint32_t)(kLdsPerCu / (total ? total : 1u));
    return n < 8u ? n : 8u;
}

// ---- per-wave LDS of the GLCM feature launches --------------------------------------------------------------------------------------
__host__ __device__ inline size_t glcm_cnt_bytes(size_t ngc) { return ((size_t)4 * kMaxAngles * ngc * ngc + 15) & ~(size_t)15; }
// glcm_features_kernel: counts [na * ngc^2] u32 | (unused) [ngc] | marginals [4][6 * ngc] | features [4][32] | sums [4][32]  (doubles)
__host__ __device__ inline size_t glcm_wave_lds(int ngc) { return glcm_cnt_bytes(ngc) + 8ull * (ngc + kMaxAngles * 6 * ngc + 2 * kMaxAngles * 32); }
// a count block of glcm_features_kernel8, at least the 1 KiB the ROI's features take in its place
__host__ __device__ inline size_t glcm8_cnt_bytes(uint32_t ngc)
{
    const size_t c = glcm_cnt_bytes(ngc), fbytes = 8ull * kMaxAngles * 32;
    return c > fbytes ? c : fbytes;
}
// glcm_features_kernel8: count blocks [2] | per group (8): pcol [8] prow [8] | sums [8][32]  (doubles) -- 5 KiB per wave at 8 levels
__host__ __device__ inline size_t glcm8_wave_lds(uint32_t ngc) { return 2 * glcm8_cnt_bytes(ngc) + 8ull * (2 * kMaxAngles * 16 + 2 * kMaxAngles * 32); }
inline size_t glcm_features_lds(uint32_t ng_cap) { return glcm_wave_lds(ng_cap) * kWaves; }
inline size_t glcm_features8_lds(uint32_t ng_cap) { return glcm8_wave_lds(ng_cap) * kWaves; }

// ---- the builds ---------------------------------------------------------------------------------------------------------------------
// A row: the template arguments of roi_features_body (GS, C16, SPLIT, D8, FAM, TIER, G16, WIN, NW, DEFER_P) and the workgroups per CU
// the build is compiled for (__launch_bounds__(NW * 64, MINWG): 8 / 7 / 6 / 5 / 4 under 64 / 72 / 80 / 96 / 128 VGPRs).
//   workspace  GS: state in a global workspace (RoiArgs::sp.scratch), LdsLayout::gs_lds_bytes of dynamic LDS; outside the opt-in
//   generic    run-time family switches, WIN = 2 (cloud or window decided per launch), tiers 4 .. 7 of a (C16, SPLIT, D8) set
//   compact    a compile-time family set (FAM 1 INTENSITY + GLCM, 2 INTENSITY, 3 GLCM) and loader (WIN), tiers 8 .. 6; the tier-8
//              builds with the intensity block leave its closing math to intensity_close_kernel (DEFER_P)
//   g16        grey depths 17 .. 64 (TIER 9): four waves, or eight (FAM 4: GLCM alone) per ROI
#define NYX_FB_GENERIC(X, C16, SPLIT, D8)                                                                                              \
    X(0, C16, SPLIT, D8, 0, 4, 0, 2, 4, 0, 4) X(0, C16, SPLIT, D8, 0, 5, 0, 2, 4, 0, 5)                                                \
    X(0, C16, SPLIT, D8, 0, 6, 0, 2, 4, 0, 6) X(0, C16, SPLIT, D8, 0, 7, 0, 2, 4, 0, 7)
#define NYX_FB_COMPACT(X, FAM, WIN)                                                                                                    \
    X(0, 1, (FAM != 2), 1, FAM, 8, 0, WIN, 4, (FAM != 3), 8) X(0, 1, (FAM != 2), 1, FAM, 7, 0, WIN, 4, 0, 7)                           \
    X(0, 1, (FAM != 2), 1, FAM, 6, 0, WIN, 4, 0, 6)
#define NYX_FB_G16(X, WIN) X(0, 1, 0, 1, 0, 9, 1, WIN, 4, 0, 4) X(0, 1, 0, 1, 4, 9, 1, WIN, 8, 0, 8)
//    X(GS, C16, SPLIT, D8, FAM, TIER, G16, WIN, NW, DEFER_P, MINWG)
#define NYX_FEATURE_BUILDS(X)                                                                                                          \
    X(1, 1, 0, 0, 0, 4, 0, 2, 4, 0, 4) X(1, 0, 0, 0, 0, 4, 0, 2, 4, 0, 4)                                                              \
    NYX_FB_GENERIC(X, 1, 1, 1) NYX_FB_GENERIC(X, 1, 1, 0) NYX_FB_GENERIC(X, 1, 0, 0) NYX_FB_GENERIC(X, 0, 1, 0) NYX_FB_GENERIC(X, 0, 0, 0) \
    NYX_FB_COMPACT(X, 1, 0) NYX_FB_COMPACT(X, 1, 1) NYX_FB_COMPACT(X, 2, 0) NYX_FB_COMPACT(X, 2, 1) NYX_FB_COMPACT(X, 3, 0) NYX_FB_COMPACT(X, 3, 1) \
    NYX_FB_G16(X, 0) NYX_FB_G16(X, 1)

struct FeatureBuild {
    bool gs, c16, split, d8;
    int fam, tier;
    bool g16;
    int win, nw;
    bool defer;
    int minwg;
};
constexpr bool operator==(const FeatureBuild& a, const FeatureBuild& b)
{
    return a.gs == b.gs && a.c16 == b.c16 && a.split == b.split && a.d8 == b.d8 && a.fam == b.fam && a.tier == b.tier && a.g16 == b.g16 &&
           a.win == b.win && a.nw == b.nw && a.defer == b.defer && a.minwg == b.minwg;
}
#define X(GS, C16, SPLIT, D8, FAM, TIER, G16, WIN, NW, DEFER_P, MINWG) {GS != 0, C16 != 0, SPLIT != 0, D8 != 0, FAM, TIER, G16 != 0, WIN, NW, DEFER_P != 0, MINWG},
constexpr FeatureBuild kFeatureBuilds[] = {NYX_FEATURE_BUILDS(X)};
#undef X
constexpr int kFeatureBuildCount = (int)(sizeof(kFeatureBuilds) / sizeof(kFeatureBuilds[0]));
static_assert(kFeatureBuildCount == 44, "2 workspace + 20 generic + 18 compact + 4 g16 builds");

// row of a build in the table, -1: no such build
constexpr int feature_build_row(const FeatureBuild& b)
{
    for (int i = 0; i < kFeatureBuildCount; i++)
        if (kFeatureBuilds[i] == b) return i;
    return -1;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------------
struct FeaturesKnobs {          // launch_roi_features fills this from knob::
    bool no_small;              // A/B knob: size class 0 on the workgroup-per-ROI kernels
    long long max_occ;          // tuning knob: cap of the occupancy tier, never below 4 (INT_MAX: none)
    bool g16_w4;                // A/B knob: four waves per ROI at grey depths 17 .. 64
    long long g16_w8_min;       // tuning knob: smallest class box (cells) for the eight-wave launch
    bool glcm_no_pairs;         // A/B knob: GLCM feature pass (<= 8 levels) one ROI per wave
};

#if defined(NYX_NO_FUSED) || defined(NYX_NO_DEFER)   // diagnostic builds close in-kernel and launch no closing kernel
constexpr bool kDeferBuilt = false;
#else
constexpr bool kDeferBuilt = true;
#endif

enum GlcmFeatureLaunch { kGlcmNone = 0, kGlcmPairs8, kGlcmGeneral };   // none | glcm_features_kernel8 | glcm_features_kernel

struct FeaturesPlan {
    // engine: the wave-per-ROI kernel of roi_small.hip (over `grid` slots), or a build of the table
    bool small, small_promised;
    FeatureBuild build;
    uint32_t grid, block, lds;  // geometry of the engine's launch (grid: rounded up to 8 under WindowSrc::xcd_swz)
    // closing launch (intensity_close_kernel): the tier-8 builds with the intensity block defer to it
    bool close, close_args_missing;   // close_args_missing: the launch defers and RoiArgs::close_rec / close_flag is null -- nothing is launched
    uint32_t close_grid;
    // GLCM feature launch over the exported counts
    GlcmFeatureLaunch glcm;
    bool glcm_all_classes;      // RoiArgs::glcm_feats == 2: the class filter is cleared for it
    uint32_t glcm_grid;
    size_t glcm_lds;
};

constexpr int kCloseBlock = 64;   // ROIs (lanes) per workgroup of intensity_close_kernel

inline FeaturesPlan plan_features_launch(const RoiArgs& a, uint32_t grid, const FeaturesKnobs& k, bool small_supported)
{
    FeaturesPlan p{};
    const bool c16 = a.L.cnt16 != 0, win = a.win.inten != nullptr;
    const bool has_int = (a.mask & NYXHIP_FAM_INTENSITY) != 0, has_glcm = (a.mask & NYXHIP_FAM_GLCM) != 0;
    p.grid = grid; p.block = kBlock; p.lds = a.L.total;
    if (a.sp.scratch) {                                   // workspace launch: nothing follows it
        p.build = FeatureBuild{true, c16, false, false, 0, 4, false, 2, 4, false, 4};
        p.lds = a.L.gs_lds_bytes;
        return p;
    }
    // the smallest size class on its own kernel: a wave per ROI (roi_small.hip).  small_class: 1 = a list / filtered launch of class 0,
    // 2 = a whole-batch launch whose stated extrema promise class 0 only
    if (a.small_class && !k.no_small && small_supported && (a.L.g16 || c16 || !has_int)) {
        p.small = true;
        p.small_promised = a.small_class == 2;
    } else if (a.L.g16) {
        // eight waves pay where the load and the sweep are long: 2821-px ROIs 23.0 -> 22.1 ns, 1009-px ROIs 18.5 -> 18.8: by the class's largest box
        const bool w8 = !has_int && !k.g16_w4 && a.L.dense_cap >= (uint32_t)k.g16_w8_min;
        p.build = FeatureBuild{false, true, false, true, w8 ? 4 : 0, 9, true, win ? 1 : 0, w8 ? 8 : 4, false, w8 ? 8 : 4};
    } else {
        // dense8 is set by the host only together with the 16-bit tables and the split; an intensity-only launch never touches
        // the GLCM code, so it can run the fully compact build (and its 64-VGPR tier) as well
        const bool d8 = a.L.dense8 != 0 || (c16 && !has_glcm);
        // the compact builds exist for the compile-time family sets only
        const bool glcm8 = a.L.dense8 && a.glcm_ws != nullptr && !a.ibsi && a.grey_depth > 0 && a.grey_depth <= 16;
        const bool int_only = has_int && !has_glcm, int_glcm = has_int && has_glcm && glcm8, glcm_only = has_glcm && !has_int && glcm8;
        const bool fam_ok = d8 && (int_only || int_glcm || glcm_only);
        // occupancy follows the carve-out: 8 / 7 / 6 / 5 / 4 workgroups per CU, the eighth for a compile-time family set only
        int occ = (int)lds_workgroups_per_cu(a.L.total);
        if (occ > 7 && !fam_ok) occ = 7;
        if (occ < 4) occ = 4;
        const long long cap = k.max_occ < 4 ? 4 : k.max_occ;
        if (occ > cap) occ = (int)cap;
        const int fam = !fam_ok || occ < 6 ? 0 : glcm_only ? 3 : int_only ? 2 : 1;
        if (fam) p.build = FeatureBuild{false, true, fam != 2, true, fam, occ, false, win ? 1 : 0, 4, occ == 8 && fam != 3, occ};
        else p.build = FeatureBuild{false, d8 || c16, d8 || a.glcm_ws != nullptr, d8, 0, occ, false, 2, 4, false, occ};
        // (what roi_features_body decides from DEFER_P: tier 8 implies a compile-time family set, C16 and an LDS launch)
        p.close = kDeferBuilt && occ == 8 && has_int;
        p.close_args_missing = p.close && !(a.close_rec && a.close_flag);
    }
    if (!p.small) {
        p.block = (uint32_t)p.build.nw * 64u;
        if (win && a.win.xcd_swz) p.grid = (grid + 7u) & ~7u;           // (xcd_slot: every XCD walks its own eighth of the slots)
    }
    if (a.L.g16)
        return p;                                         // features inside the kernel, nothing deferred
    p.close_grid = (grid + kCloseBlock - 1) / kCloseBlock;              // (the follow-up launches run over the same slots)
    if (a.glcm_ws != nullptr && a.glcm_feats != 1) {
        // eight lanes per angle, two ROIs per wave up to 8 levels
        p.glcm = a.L.ng_cap <= 8 && !k.glcm_no_pairs ? kGlcmPairs8 : kGlcmGeneral;
        p.glcm_all_classes = a.glcm_feats == 2;   // (the class-0 group of this call left its counts for this launch: everybody with a matrix order is derived)
        p.glcm_grid = p.glcm == kGlcmPairs8 ? (grid + 2 * kWaves - 1) / (2 * kWaves) : (grid + kWaves - 1) / kWaves;
        p.glcm_lds = p.glcm == kGlcmPairs8 ? glcm_features8_lds(a.L.ng_cap) : glcm_features_lds(a.L.ng_cap);
    }
    return p;
}

} // namespace nyxhip
