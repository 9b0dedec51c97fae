// plan_features_launch / NYX_FEATURE_BUILDS of nyxus_amd/csrc/features_plan.h on the host alone (no HIP, no library, no environment;
// the device qualifiers of roi_kernel.h are defined away).
//   1. the oracle: the selection chain the launcher had before the table (launch_roi_features + launch_lds_variant, one `if` per
//      hipLaunchKernelGGL), transcribed to return what it would launch -- the wrapper as the template arguments and launch bounds that
//      wrapper gave the body.  The plan agrees with it on every point of the grid below (the full cross product).
//   2. every build a plan names is a row of the table; rows no grid point reaches are printed (reported, not failed).
//   3. literal rows: the benchmark configuration at every occupancy cap, a g16w8 row, a workspace row.
// Prints "ALL PASSED"; exit code 1 on a failure.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
struct uint2 { unsigned x, y; };       // (roi_kernel.h names the HIP vector type in launch-argument structs)
#include "../../nyxus_amd/csrc/features_plan.h"

using namespace nyxhip;

// ---- the oracle ------------------------------------------------------------------------------------------------------------------------
struct Launch {
    bool small, promised;
    FeatureBuild b;
    uint32_t grid, block, lds;
    bool invalid;                      // hipErrorInvalidValue in front of any launch
    bool close; uint32_t close_grid;
    int glcm; uint32_t glcm_grid; size_t glcm_lds; bool glcm_all;
};

// the nine wrappers: what each passed to roi_features_body, and its __launch_bounds__
static FeatureBuild w_base(bool gs, bool c16, bool split, bool d8) { return {gs, c16, split, d8, 0, 4, false, 2, 4, false, 4}; }   // roi_features_kernel<GS, C16, SPLIT, D8>
static FeatureBuild w_occ(int t, bool c16, bool split, bool d8) { return {false, c16, split, d8, 0, t, false, 2, 4, false, t}; }    // _occ5 / _occ6 / _occ7
static FeatureBuild w_occ8(int fam, int win) { return {false, true, fam == 1 || fam == 3, true, fam, 8, false, win, 4, fam == 1 || fam == 2, 8}; }
static FeatureBuild w_fam(int t, int fam, int win) { return {false, true, fam == 1 || fam == 3, true, fam, t, false, win, 4, false, t}; }   // _fam7 / _fam6
static FeatureBuild w_g16(int win) { return {false, true, false, true, 0, 9, true, win, 4, false, 4}; }
static FeatureBuild w_g16w8(int win) { return {false, true, false, true, 4, 9, true, win, 8, false, 8}; }

static size_t o_glcm_features8_lds(uint32_t ng_cap)
{
    const size_t c = ((size_t)4 * kMaxAngles * ng_cap * ng_cap + 15) & ~(size_t)15, fbytes = 8ull * kMaxAngles * 32;
    return (2 * (c > fbytes ? c : fbytes) + 8ull * (2 * kMaxAngles * 16 + 2 * kMaxAngles * 32)) * kWaves;
}
static size_t o_glcm_features_lds(uint32_t ng_cap)
{
    const size_t per_wave = (((size_t)4 * kMaxAngles * ng_cap * ng_cap + 15) & ~(size_t)15) + 8ull * (ng_cap + kMaxAngles * 6 * ng_cap + 2 * kMaxAngles * 32);
    return per_wave * kWaves;
}
static int o_cap_occ(int occ, long long max_occ) { const long long v = max_occ, cap = v < 4 ? 4 : v; return occ < cap ? occ : (int)cap; }

static void o_lds_variant(bool C16, bool SPLIT, bool D8, const RoiArgs& a, uint32_t grid, const FeaturesKnobs& k, bool& deferred, Launch& L)
{
    deferred = false;
    const size_t lds = 160 * 1024;
    const bool int_only = !(a.mask & NYXHIP_FAM_GLCM) && (a.mask & NYXHIP_FAM_INTENSITY);
    const bool int_glcm = (a.mask & NYXHIP_FAM_GLCM) && (a.mask & NYXHIP_FAM_INTENSITY) && a.L.dense8 && a.glcm_ws != nullptr && !a.ibsi &&
                          a.grey_depth > 0 && a.grey_depth <= 16;
    const bool glcm_only = (a.mask & NYXHIP_FAM_GLCM) && !(a.mask & NYXHIP_FAM_INTENSITY) && a.L.dense8 && a.glcm_ws != nullptr && !a.ibsi &&
                           a.grey_depth > 0 && a.grey_depth <= 16;
    const bool fam_ok = C16 && SPLIT && D8 && (int_only || int_glcm || glcm_only);
    int occ = 4;
    for (int o = fam_ok ? 8 : 7; o > 4; o--)
        if ((size_t)o * a.L.total <= lds) { occ = o; break; }
    occ = o_cap_occ(occ, k.max_occ);
    const bool win = a.win.inten != nullptr;
    if (win && a.win.xcd_swz) grid = (grid + 7u) & ~7u;
    deferred = occ == 8 && (a.mask & NYXHIP_FAM_INTENSITY) != 0;
    if (deferred && !(a.close_rec && a.close_flag)) { L.invalid = true; return; }
    L.grid = grid; L.block = kBlock; L.lds = a.L.total;
    if (fam_ok && glcm_only && occ >= 6) {
        if (occ == 8) { if (win) L.b = w_occ8(3, 1); else L.b = w_occ8(3, 0); }
        else if (occ == 7) { if (win) L.b = w_fam(7, 3, 1); else L.b = w_fam(7, 3, 0); }
        else { if (win) L.b = w_fam(6, 3, 1); else L.b = w_fam(6, 3, 0); }
    }
    else if (occ == 8 && int_only && win) L.b = w_occ8(2, 1);
    else if (occ == 8 && int_only) L.b = w_occ8(2, 0);
    else if (occ == 8 && win) L.b = w_occ8(1, 1);
    else if (occ == 8) L.b = w_occ8(1, 0);
    else if (fam_ok && occ == 7 && int_only && win) L.b = w_fam(7, 2, 1);
    else if (fam_ok && occ == 7 && int_only) L.b = w_fam(7, 2, 0);
    else if (fam_ok && occ == 7 && win) L.b = w_fam(7, 1, 1);
    else if (fam_ok && occ == 7) L.b = w_fam(7, 1, 0);
    else if (fam_ok && occ == 6 && int_only && win) L.b = w_fam(6, 2, 1);
    else if (fam_ok && occ == 6 && int_only) L.b = w_fam(6, 2, 0);
    else if (fam_ok && occ == 6 && win) L.b = w_fam(6, 1, 1);
    else if (fam_ok && occ == 6) L.b = w_fam(6, 1, 0);
    else if (occ == 7) L.b = w_occ(7, C16, SPLIT, D8);
    else if (occ == 6) L.b = w_occ(6, C16, SPLIT, D8);
    else if (occ == 5) L.b = w_occ(5, C16, SPLIT, D8);
    else L.b = w_base(false, C16, SPLIT, D8);
}

static Launch oracle(const RoiArgs& a, uint32_t grid, const FeaturesKnobs& k, bool small_supported)
{
    Launch L;
    memset(&L, 0, sizeof(L));
    const bool c16 = a.L.cnt16 != 0;
    if (a.sp.scratch) {
        L.grid = grid; L.block = kBlock; L.lds = a.L.gs_lds_bytes;
        if (c16) L.b = w_base(true, true, false, false);
        else L.b = w_base(true, false, false, false);
        return L;
    }
    const bool no_small = k.no_small;
    if (a.L.g16) {
        if (a.small_class && !no_small && small_supported) { L.small = true; L.grid = grid; L.promised = a.small_class == 2; return L; }
        L.lds = a.L.total;
        if (!(a.mask & NYXHIP_FAM_INTENSITY) && !k.g16_w4 && a.L.dense_cap >= (uint32_t)k.g16_w8_min) {
            L.block = 512;
            if (a.win.inten != nullptr) { L.b = w_g16w8(1); L.grid = a.win.xcd_swz ? (grid + 7u) & ~7u : grid; }
            else { L.b = w_g16w8(0); L.grid = grid; }
        } else {
            L.block = kBlock;
            if (a.win.inten != nullptr) { L.b = w_g16(1); L.grid = a.win.xcd_swz ? (grid + 7u) & ~7u : grid; }
            else { L.b = w_g16(0); L.grid = grid; }
        }
        return L;
    }
    const bool split = a.glcm_ws != nullptr;
    const bool d8 = a.L.dense8 != 0 || (c16 && !(a.mask & NYXHIP_FAM_GLCM));
    bool deferred = false;
    if (a.small_class && !no_small && (c16 || !(a.mask & NYXHIP_FAM_INTENSITY)) && small_supported) { L.small = true; L.grid = grid; L.promised = a.small_class == 2; }
    else if (d8) o_lds_variant(true, true, true, a, grid, k, deferred, L);
    else if (c16) { if (split) o_lds_variant(true, true, false, a, grid, k, deferred, L); else o_lds_variant(true, false, false, a, grid, k, deferred, L); }
    else { if (split) o_lds_variant(false, true, false, a, grid, k, deferred, L); else o_lds_variant(false, false, false, a, grid, k, deferred, L); }
    if (L.invalid) return L;
    if (deferred) { L.close = true; L.close_grid = (grid + 64 - 1) / 64; }
    if (split && a.glcm_feats != 1) {
        L.glcm_all = a.glcm_feats == 2;
        if (a.L.ng_cap <= 8 && !k.glcm_no_pairs) { L.glcm = 1; L.glcm_grid = (grid + 2 * kWaves - 1) / (2 * kWaves); L.glcm_lds = o_glcm_features8_lds(a.L.ng_cap); }
        else { L.glcm = 2; L.glcm_grid = (grid + kWaves - 1) / kWaves; L.glcm_lds = o_glcm_features_lds(a.L.ng_cap); }
    }
    return L;
}

// ---- plan against oracle ---------------------------------------------------------------------------------------------------------------
static bool agree(const FeaturesPlan& p, const Launch& L)
{
    if (L.invalid) return p.close_args_missing;
    if (p.close_args_missing) return false;
    if (p.small != L.small || p.grid != L.grid) return false;
    if (p.small ? p.small_promised != L.promised : !(p.build == L.b) || p.block != L.block || p.lds != L.lds) return false;
    if (p.close != L.close || (p.close && p.close_grid != L.close_grid)) return false;
    if ((int)p.glcm != L.glcm) return false;
    return p.glcm == kGlcmNone || (p.glcm_grid == L.glcm_grid && p.glcm_lds == L.glcm_lds && p.glcm_all_classes == L.glcm_all);
}

static const uint32_t kMasks[] = {1, 2, 3};
static const int kDepths[] = {-16, 8, 16, 17, 64, 100};
static const uint32_t kTotals[] = {20480, 20481, 23405, 23406, 27306, 27307, 32768, 32769, 40960};   // both sides of 160 KiB / 8, / 7, / 6, / 5
static const long long kMaxOcc[] = {INT_MAX, 3, 4, 5, 6, 7, 8};
static const uint32_t kDenseCaps[] = {2303, 2304};
static const uint32_t kNgCaps[] = {8, 9, 16};
static const uint32_t kGrids[] = {1, 7, 8, 9, 64, 65};

struct Tally { unsigned long long points = 0, bad = 0, untabled = 0; unsigned long long hit[kFeatureBuildCount] = {}; char first[256] = ""; };

static void walk(uint32_t mask, uint32_t total, Tally& T)
{
    static uint32_t ws_word, flag_word, some;
    static double rec_word;
    static unsigned char scratch_byte;
    RoiArgs a;
    memset(&a, 0, sizeof(a));
    a.mask = mask; a.L.total = total; a.L.gs_lds_bytes = 4096;
    FeaturesKnobs k;
    k.g16_w8_min = 2304;
    for (int cnt16 = 0; cnt16 < 2; cnt16++) { a.L.cnt16 = cnt16;
    for (int ws = 0; ws < 2; ws++) { a.glcm_ws = ws ? &ws_word : nullptr;
    for (int d8 = 0; d8 < 2; d8++) { a.L.dense8 = d8;
    for (int g16 = 0; g16 < 2; g16++) { a.L.g16 = g16;
    for (int ibsi = 0; ibsi < 2; ibsi++) { a.ibsi = ibsi;
    for (int gd : kDepths) { a.grey_depth = gd;
    for (int scr = 0; scr < 2; scr++) { a.sp.scratch = scr ? &scratch_byte : nullptr;
    for (int win = 0; win < 3; win++) { a.win.inten = win ? &some : nullptr; a.win.xcd_swz = win == 2;      // none | set | set under xcd_swz
    for (uint32_t sc = 0; sc < 3; sc++) { a.small_class = sc;
    for (int sup = 0; sup < 2; sup++)
    for (int ns = 0; ns < 2; ns++) { k.no_small = ns;
    for (long long mo : kMaxOcc) { k.max_occ = mo;
    for (int w4 = 0; w4 < 2; w4++) { k.g16_w4 = w4;
    for (uint32_t dc : kDenseCaps) { a.L.dense_cap = dc;
    for (uint32_t ngc : kNgCaps) { a.L.ng_cap = ngc;
    for (int np = 0; np < 2; np++) { k.glcm_no_pairs = np;
    for (uint32_t gf = 0; gf < 3; gf++) { a.glcm_feats = gf;
    for (int cl = 0; cl < 2; cl++) { a.close_rec = &rec_word; a.close_flag = cl ? nullptr : &flag_word;      // both set | one missing
    for (uint32_t grid : kGrids) {
        const FeaturesPlan p = plan_features_launch(a, grid, k, sup != 0);
        const Launch L = oracle(a, grid, k, sup != 0);
        T.points++;
        if (!agree(p, L)) {
            if (!T.bad++)
                snprintf(T.first, sizeof(T.first), "mask %u total %u cnt16 %d ws %d dense8 %d g16 %d ibsi %d gd %d scratch %d win %d small_class %u supported %d no_small %d "
                         "max_occ %lld w4 %d dense_cap %u ng_cap %u no_pairs %d glcm_feats %u close %d grid %u", mask, total, cnt16, ws, d8, g16, ibsi, gd, scr, win, sc, sup, ns,
                         mo, w4, dc, ngc, np, gf, cl, grid);
        }
        if (!p.small && !p.close_args_missing) {
            const int row = feature_build_row(p.build);
            if (row < 0) T.untabled++; else T.hit[row]++;
        }
    }}}}}}}}}}}}}}}}}}
}

static int g_bad = 0;
static void expect(bool ok, const char* what)
{
    printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) g_bad++;
}

static void literal_rows()
{
    static uint32_t ws_word, flag_word;
    static double rec_word;
    static unsigned char scratch_byte;
    const FeaturesKnobs dflt = {false, INT_MAX, false, 48 * 48, false};
    // the benchmark configuration: INTENSITY + GLCM at grey depth 8, a 20192-byte carve-out, clouds
    RoiArgs a;
    memset(&a, 0, sizeof(a));
    a.mask = 3; a.grey_depth = 8; a.L.total = 20192; a.L.cnt16 = 1; a.L.dense8 = 1; a.L.ng_cap = 8; a.glcm_ws = &ws_word; a.close_rec = &rec_word; a.close_flag = &flag_word;
    const uint32_t n = 196000;
    FeaturesPlan p = plan_features_launch(a, n, dflt, false);
    expect(!p.small && p.build == FeatureBuild{false, true, true, true, 1, 8, false, 0, 4, true, 8} && p.grid == n && p.block == 256 && p.lds == 20192,
           "benchmark: tier 8, FAM 1, WIN 0, deferred");
    expect(p.close && !p.close_args_missing && p.close_grid == (n + 63) / 64, "benchmark: the closing launch follows over ceil(n / 64) workgroups");
    expect(p.glcm == kGlcmPairs8 && p.glcm_grid == (n + 7) / 8 && p.glcm_lds == 4 * 5120 && !p.glcm_all_classes, "benchmark: the 8-level GLCM launch follows over ceil(n / 8) workgroups");
    for (int cap = 7; cap >= 4; cap--) {
        FeaturesKnobs k = dflt;
        k.max_occ = cap;
        p = plan_features_launch(a, n, k, false);
        const FeatureBuild want = cap >= 6 ? FeatureBuild{false, true, true, true, 1, cap, false, 0, 4, false, cap} : FeatureBuild{false, true, true, true, 0, cap, false, 2, 4, false, cap};
        char what[96];
        snprintf(what, sizeof(what), "benchmark under max_occ %d: tier %d, FAM %d, closes in the kernel", cap, cap, cap >= 6 ? 1 : 0);
        expect(p.build == want && !p.close && p.glcm == kGlcmPairs8 && p.lds == 20192, what);
    }
    // grey depth 64, GLCM alone, a class box of 48 x 48: eight waves per ROI; one cell less: four
    RoiArgs g;
    memset(&g, 0, sizeof(g));
    g.mask = 2; g.grey_depth = 64; g.L.g16 = 1; g.L.cnt16 = 1; g.L.total = 39800; g.L.dense_cap = 2304; g.L.ng_cap = 64;
    p = plan_features_launch(g, 9, dflt, false);
    expect(p.build == FeatureBuild{false, true, false, true, 4, 9, true, 0, 8, false, 8} && p.block == 512 && p.grid == 9 && p.lds == 39800 && !p.close && p.glcm == kGlcmNone,
           "g16w8: FAM 4, TIER 9, eight waves, 512 threads");
    g.L.dense_cap = 2303;
    p = plan_features_launch(g, 9, dflt, false);
    expect(p.build == FeatureBuild{false, true, false, true, 0, 9, true, 0, 4, false, 4} && p.block == 256, "g16: four waves below the eight-wave box");
    // a workspace launch
    a.sp.scratch = &scratch_byte; a.L.gs_lds_bytes = 12288;
    p = plan_features_launch(a, 5, dflt, true);
    expect(!p.small && p.build == FeatureBuild{true, true, false, false, 0, 4, false, 2, 4, false, 4} && p.lds == 12288 && p.grid == 5 && !p.close && p.glcm == kGlcmNone,
           "workspace: the GS build on gs_lds_bytes, nothing follows");
    // the occupancy rule
    expect(lds_workgroups_per_cu(20480) == 8 && lds_workgroups_per_cu(20481) == 7 && lds_workgroups_per_cu(0) == 8 && lds_workgroups_per_cu(163840) == 1 && lds_workgroups_per_cu(163841) == 0,
           "lds_workgroups_per_cu: min(8, 160 KiB / total)");
    expect(glcm_features8_lds(8) == o_glcm_features8_lds(8) && glcm_features_lds(16) == o_glcm_features_lds(16) && glcm_features8_lds(8) == 20480, "GLCM feature launches: LDS bytes");
}

int main()
{
    // the table itself
    int dup = 0;
    for (int i = 0; i < kFeatureBuildCount; i++)
        for (int j = i + 1; j < kFeatureBuildCount; j++)
            if (kFeatureBuilds[i] == kFeatureBuilds[j]) dup++;
    expect(kFeatureBuildCount == 44 && dup == 0, "table: 44 distinct builds");

    std::vector<Tally> tallies(sizeof(kMasks) / sizeof(kMasks[0]) * sizeof(kTotals) / sizeof(kTotals[0]));
    std::vector<std::thread> pool;
    size_t t = 0;
    for (uint32_t mask : kMasks)
        for (uint32_t total : kTotals) {
            Tally* T = &tallies[t++];
            pool.emplace_back([=] { walk(mask, total, *T); });
        }
    for (auto& th : pool) th.join();
    Tally sum;
    for (const Tally& T : tallies) {
        sum.points += T.points; sum.bad += T.bad; sum.untabled += T.untabled;
        for (int i = 0; i < kFeatureBuildCount; i++) sum.hit[i] += T.hit[i];
        if (T.bad && !sum.first[0]) memcpy(sum.first, T.first, sizeof(sum.first));
    }
    printf("%s plan == oracle on %llu grid points", sum.bad ? "FAIL" : "ok  ", sum.points);
    if (sum.bad) { printf(": %llu differ, first at %s", sum.bad, sum.first); g_bad++; }
    printf("\n");
    expect(sum.untabled == 0, "every build a plan names is a row of the table");
    int unreached = 0;
    for (int i = 0; i < kFeatureBuildCount; i++)
        if (!sum.hit[i]) {
            const FeatureBuild& b = kFeatureBuilds[i];
            printf("     no grid point reaches row %d: gs %d c16 %d split %d d8 %d fam %d tier %d g16 %d win %d nw %d defer %d minwg %d\n", i, b.gs, b.c16, b.split, b.d8, b.fam, b.tier,
                   b.g16, b.win, b.nw, b.defer, b.minwg);
            unreached++;
        }
    printf("     rows reached: %d of %d\n", kFeatureBuildCount - unreached, kFeatureBuildCount);
    literal_rows();
    if (g_bad) { printf("%d FAILED\n", g_bad); return 1; }
    printf("ALL PASSED\n");
    return 0;
}
