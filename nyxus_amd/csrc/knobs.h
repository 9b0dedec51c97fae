// knobs.h -- the register of the library's NYXHIP_* environment knobs (internal; plain C++, no HIP header: tests/cpp/test_knobs.cpp).
// Every knob is a row of the table below and is read through its accessor, knob::<accessor>(); nothing else looks at the environment.
//   flag:    on if and only if the variable is set, non-empty and its first character is not '0'
//   integer: atoll of the value; the default when the variable is unset or empty
//   process: read once, with every other such knob, at the first nyxhip_init (or the first use) -- later changes are not seen
//   call:    read from the environment at every use (the tests flip these between calls on one context)
// What a knob does to a result, and what was measured with it, is told in INTEGRATION.md section 4 and at its call site.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdlib.h>
#include <type_traits>

namespace nyxhip {
namespace knob {

enum Kind { flag, integer };
enum When { process, call };

//    accessor, NYXHIP_<name>, kind, read, default, meaning
#define NYXHIP_KNOB_TABLE(X)                                                                                                           \
    X(debug, DEBUG, flag, call, 0, "one line per launch on stderr")                                                                    \
    X(dep_seq, DEP_SEQ, flag, call, 0, "dependence tails one after the other on one wave")                                             \
    X(g16_fused, G16_FUSED, flag, call, 0, "INTENSITY + GLCM at grey depths 17..64 in one launch")                                     \
    X(no_coop_gabor, NO_COOP_GABOR, flag, call, 0, "GABOR beyond LDS: one workgroup per ROI")                                          \
    X(max_occ, MAX_OCC, integer, call, INT_MAX, "cap of roi_features_kernel's occupancy tier, never below 4 (cap_occ)")               \
    X(large_budget_mb, LARGE_BUDGET_MB, integer, call, 0, "MiB of workspace of a large-ROI path or deferred list (large_budget)")     \
    X(large_dbg, LARGE_DBG, integer, call, 0, "diagnostic: phases the several-workgroups path leaves out (bits)")                     \
    X(no_mom_lane, NO_MOM_LANE, flag, process, 0, "contour + moments chain on the call's stream")                                      \
    X(no_window, NO_WINDOW, flag, process, 0, "tile path: always materialise ROI clouds")                                              \
    X(no_xcd_swizzle, NO_XCD_SWIZZLE, flag, process, 0, "tile path: workgroup b of a window launch serves ROI b")                      \
    X(no_staging, NO_STAGING, flag, process, 0, "host stacks through the runtime's pageable copy")                                     \
    X(no_pin, NO_PIN, flag, process, 0, "own-mapping host stacks are not registered")                                                  \
    X(ih_one_form, IH_ONE_FORM, flag, process, 0, "intensity histogram: every ROI through the workgroup form")                         \
    X(no_small, NO_SMALL, flag, process, 0, "size class 0 on the workgroup-per-ROI kernels")                                           \
    X(g16_w4, G16_W4, flag, process, 0, "GLCM at grey depths 17..64 on four waves per ROI for every class")                            \
    X(glcm_no_pairs, GLCM_NO_PAIRS, flag, process, 0, "GLCM feature pass (<= 8 levels): one ROI per wave")                             \
    X(gabor_no_lpsep, GABOR_NO_LPSEP, flag, process, 0, "Gabor low-pass screening as the full 256-tap pass")                           \
    X(lds_lanes, LDS_LANES, flag, process, 0, "every LDS size class of an exact call on a stream of its own")                          \
    X(no_coop, NO_COOP, flag, process, 0, "ROIs beyond LDS: one workgroup per ROI (INTENSITY / GLCM and texture)")                     \
    X(no_coop_tex, NO_COOP_TEX, flag, process, 0, "ROIs beyond LDS: texture families one workgroup per ROI")                           \
    X(no_coop_tex_sc2, NO_COOP_TEX_SC2, flag, process, 0, "size class 2: texture families one workgroup per ROI (no_sc2_tex)")         \
    X(no_wide, NO_WIDE, flag, process, 0, "16-bit ranges through the sort engine of the fused kernel")                                 \
    X(no_gabor_lane, NO_GABOR_LANE, flag, process, 0, "size class 2's Gabor launch on the call's stream")                              \
    X(no_lanes, NO_LANES, flag, process, 0, "large size classes on the context's stream")                                              \
    X(no_dep_lane, NO_DEP_LANE, flag, process, 0, "dependence trio of a large class on the class's stream")                            \
    X(class_sync, CLASS_SYNC, flag, process, 0, "always the classifier + exact per-class launches")                                    \
    X(no_adapt, NO_ADAPT, flag, process, 0, "never switch to exact class lists on the census of recent calls")                         \
    X(no_merge_large, NO_MERGE_LARGE, flag, process, 0, "the size classes beyond LDS as a launch group each")                        \
    X(no_lane_priority, NO_LANE_PRIORITY, flag, process, 0, "lane streams at the default priority")                                    \
    X(gabor_fused, GABOR_FUSED, flag, process, 0, "Gabor: fused taps, decisions unchecked (gabor_mode 1)")                             \
    X(gabor_exact, GABOR_EXACT, flag, process, 0, "Gabor: the reference's arithmetic throughout (gabor_mode 0)")                       \
    X(stamps, STAMPS, flag, process, 0, "-DNYX_STAMP builds: per-phase cycle sums at nyxhip_destroy")                                  \
    X(g16_w8_min, G16_W8_MIN, integer, process, 48 * 48, "smallest class box (cells) for the eight-wave GLCM launch")                  \
    X(mom_occ, MOM_OCC, integer, process, 6, "cap of roi_moments_kernel's occupancy tier")                                             \
    X(tex_occ, TEX_OCC, integer, process, 8, "cap of roi_texture_kernel's occupancy tier")                                             \
    X(dbg_phase, DBG_PHASE, integer, process, 0, "-DNYXHIP_GABOR_PHASE_EXITS builds: phase a Gabor workgroup leaves after")            \
    X(gabor_mode_env, GABOR_MODE, integer, process, 4, "Gabor kernel generation 2 or 3, else 4 (gabor_mode)")

struct Row { const char* name; Kind kind; When when; long long dflt; const char* meaning; };
#define X(fn, NAME, kind, when, dflt, meaning) {"NYXHIP_" #NAME, kind, when, dflt, meaning},
constexpr Row kTable[] = {NYXHIP_KNOB_TABLE(X)};
#undef X
#define X(fn, NAME, kind, when, dflt, meaning) k_##fn,
enum { NYXHIP_KNOB_TABLE(X) kCount };
#undef X

// the one place that reads the environment
inline long long read(int i)
{
    const char* e = getenv(kTable[i].name);
    if (!e || !*e) return kTable[i].dflt;
    return kTable[i].kind == flag ? *e != '0' : atoll(e);
}

// the table as the first nyxhip_init met it (initialised once, whichever thread comes first; the `call` rows are not served from it)
struct AtStart { long long v[kCount]; };
inline const AtStart& at_start()
{
    static const AtStart s = [] { AtStart r; for (int i = 0; i < kCount; i++) r.v[i] = read(i); return r; }();
    return s;
}

#define X(fn, NAME, kind, when, dflt, meaning)                                                                                         \
    inline std::conditional_t<kind == flag, bool, long long> fn()                                                                      \
    { return static_cast<std::conditional_t<kind == flag, bool, long long>>(when == call ? read(k_##fn) : at_start().v[k_##fn]); }
NYXHIP_KNOB_TABLE(X)
#undef X

// ---- derived values ----------------------------------------------------------------------------------------------------------------
// occupancy tier `occ` of roi_features_kernel under NYXHIP_MAX_OCC: min(occ, max(knob, 4))
inline int cap_occ(int occ) { const long long v = max_occ(), cap = v < 4 ? 4 : v; return occ < cap ? occ : (int)cap; }
// workspace budget in bytes: NYXHIP_LARGE_BUDGET_MB when it is > 0 (tests: a small budget sends a class, or a list, through the
// chunked form), else the path's default
inline size_t large_budget(size_t dflt) { const long long mb = large_budget_mb(); return mb > 0 ? (size_t)mb << 20 : dflt; }
// the tiled Gabor kernel's variant: NYXHIP_GABOR_FUSED > NYXHIP_GABOR_EXACT > NYXHIP_GABOR_MODE
inline int gabor_mode() { const long long m = gabor_mode_env(); return gabor_fused() ? 1 : gabor_exact() ? 0 : (m == 2 || m == 3) ? (int)m : 4; }
// size class 2 keeps its texture families on the one-workgroup path
inline bool no_sc2_tex() { return no_coop_tex_sc2() || no_coop_tex() || no_coop(); }

} // namespace knob
} // namespace nyxhip
