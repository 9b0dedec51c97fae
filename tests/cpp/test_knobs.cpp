// nyxus_amd/csrc/knobs.h on the host alone (no HIP, no library): the flag rule, the two read times, the integers and the derived values.
//   (no argument)  the checks one process can make: one line per check and "ALL PASSED"; exit code 1 when one fails
//   --list         one line per table row: name, kind, read time
//   --start        one line per accessor and derived value as this process's environment gives them (the per-process knobs are
//                  read once, so tests/test_knobs_cpu.py starts a process per start-up environment)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../nyxus_amd/csrc/knobs.h"

namespace knob = nyxhip::knob;

static int g_bad = 0;

static void expect(const char* what, const char* value, long long got, long long want)
{
    const bool ok = got == want;
    printf("%s %s [%s]: %lld (want %lld)\n", ok ? "ok  " : "FAIL", what, value ? value : "unset", got, want);
    if (!ok) g_bad++;
}

static void put(const char* name, const char* value)
{
    if (value) setenv(name, value, 1);
    else unsetenv(name);
}

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--list")) {
        for (const knob::Row& r : knob::kTable)
            printf("%s %s %s\n", r.name, r.kind == knob::flag ? "flag" : "integer", r.when == knob::call ? "call" : "process");
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "--start")) {
#define X(fn, NAME, kind, when, dflt, meaning) printf("%s %lld\n", #fn, (long long)knob::fn());
        NYXHIP_KNOB_TABLE(X)
#undef X
        printf("gabor_mode %d\nno_sc2_tex %d\n", knob::gabor_mode(), (int)knob::no_sc2_tex());
        return 0;
    }
    for (const knob::Row& r : knob::kTable) unsetenv(r.name);

    // ---- per process: the defaults, and deaf to the environment after the first read
    expect("no_small at start", nullptr, knob::no_small(), 0);
    expect("g16_w8_min default", nullptr, knob::g16_w8_min(), 2304);
    expect("mom_occ default", nullptr, knob::mom_occ(), 6);
    expect("tex_occ default", nullptr, knob::tex_occ(), 8);
    expect("dbg_phase default", nullptr, knob::dbg_phase(), 0);
    expect("gabor_mode default", nullptr, knob::gabor_mode(), 4);
    expect("no_sc2_tex default", nullptr, knob::no_sc2_tex(), 0);
    put("NYXHIP_NO_SMALL", "1"); put("NYXHIP_TEX_OCC", "4"); put("NYXHIP_GABOR_FUSED", "1"); put("NYXHIP_NO_COOP", "1");
    expect("no_small after the first read", "1", knob::no_small(), 0);
    expect("tex_occ after the first read", "4", knob::tex_occ(), 8);
    expect("gabor_mode after the first read", "1", knob::gabor_mode(), 4);
    expect("no_sc2_tex after the first read", "1", knob::no_sc2_tex(), 0);

    // ---- per call: the flag rule, and every read follows the environment
    const struct { const char* value; int on; } rule[] = {{nullptr, 0}, {"", 0}, {"0", 0}, {"00", 0}, {"01", 0}, {"1", 1}, {"yes", 1}};
    for (const auto& c : rule) {
        put("NYXHIP_DEP_SEQ", c.value);
        expect("dep_seq", c.value, knob::dep_seq(), c.on);
    }
    put("NYXHIP_DEBUG", "1");
    expect("debug, set", "1", knob::debug(), 1);
    put("NYXHIP_DEBUG", nullptr);
    expect("debug, removed again", nullptr, knob::debug(), 0);
    put("NYXHIP_G16_FUSED", "0"); put("NYXHIP_NO_COOP_GABOR", "1");
    expect("g16_fused", "0", knob::g16_fused(), 0);
    expect("no_coop_gabor", "1", knob::no_coop_gabor(), 1);

    // ---- per call integers: default, empty string, value
    expect("large_dbg", nullptr, knob::large_dbg(), 0);
    put("NYXHIP_LARGE_DBG", "");
    expect("large_dbg", "", knob::large_dbg(), 0);
    put("NYXHIP_LARGE_DBG", "5");
    expect("large_dbg", "5", knob::large_dbg(), 5);
    const struct { const char* value; int occ; } cap[] = {{nullptr, 7}, {"", 7}, {"3", 4}, {"4", 4}, {"6", 6}, {"9", 7}, {"0", 4}};
    for (const auto& c : cap) {
        put("NYXHIP_MAX_OCC", c.value);
        expect("cap_occ(7) under max_occ", c.value, knob::cap_occ(7), c.occ);
    }
    put("NYXHIP_MAX_OCC", "6");
    expect("cap_occ(4) under max_occ", "6", knob::cap_occ(4), 4);
    const long long dflt = 8ll << 30;
    const struct { const char* value; long long bytes; } budget[] = {{nullptr, dflt}, {"", dflt}, {"0", dflt}, {"-1", dflt}, {"x", dflt},
                                                                     {"2", 2ll << 20}, {"16384", 16384ll << 20}};
    for (const auto& c : budget) {
        put("NYXHIP_LARGE_BUDGET_MB", c.value);
        expect("large_budget(8 GiB)", c.value, (long long)knob::large_budget((size_t)dflt), c.bytes);
    }
    if (g_bad) { printf("%d FAILED\n", g_bad); return 1; }
    printf("ALL PASSED\n");
    return 0;
}
