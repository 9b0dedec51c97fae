// glcm_row_bounds / glcm_row_bounds_even of nyxus_amd/csrc/roi_kernel.h: the row blocks the four waves of a workgroup take in the
// co-occurrence sweep, on the host alone (no HIP, no library; the header's device qualifiers are defined away).  For every box
// height 1 .. 8192: the bounds start at 0, end at h, never fall, and the four blocks cover each row exactly once; the blocks of
// waves 2 and 3 of the weighted form are non-empty once h >= 4.  Prints a line per form and "ALL PASSED"; exit code 1 on a failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
struct uint2 { unsigned x, y; };       // (the header names the HIP vector type in launch-argument structs)
#include "../../nyxus_amd/csrc/roi_kernel.h"

static int g_bad = 0;

template <class F>
static void walk(const char* what, F bounds, bool weighted)
{
    uint32_t first_bad = 0;
    const char* why = "";
    for (uint32_t h = 1; h <= 8192 && !first_bad; h++) {
        uint32_t b[5];
        for (uint32_t k = 0; k <= 4; k++) b[k] = bounds(h, k);
        if (b[0] != 0) { first_bad = h; why = "does not start at 0"; break; }
        if (b[4] != h) { first_bad = h; why = "does not end at h"; break; }
        for (int k = 0; k < 4; k++)
            if (b[k] > b[k + 1]) { first_bad = h; why = "not monotone"; }
        if (first_bad) break;
        std::vector<unsigned char> seen(h, 0);
        for (int k = 0; k < 4; k++)
            for (uint32_t r = b[k]; r < b[k + 1]; r++) {
                if (r >= h || seen[r]) { first_bad = h; why = "a row twice or beyond the box"; break; }
                seen[r] = 1;
            }
        for (uint32_t r = 0; r < h && !first_bad; r++)
            if (!seen[r]) { first_bad = h; why = "a row left out"; }
        if (!first_bad && weighted && h >= 4 && (b[2] == b[3] || b[3] == b[4])) { first_bad = h; why = "wave 2 or 3 without a row"; }
    }
    printf("%s %s: heights 1 .. 8192%s%s", first_bad ? "FAIL" : "ok  ", what, first_bad ? ", first at h = " : "", first_bad ? "" : "\n");
    if (first_bad) { printf("%u (%s)\n", first_bad, why); g_bad++; }
}

int main()
{
    walk("glcm_row_bounds", [](uint32_t h, uint32_t k) { return nyxhip::glcm_row_bounds(h, k); }, true);
    walk("glcm_row_bounds_even", [](uint32_t h, uint32_t k) { return nyxhip::glcm_row_bounds_even(h, k); }, false);
    // the equal blocks are the ones the serial order always had: ceil(h / 4) rows a wave, the last ones short or empty
    int same = 1;
    for (uint32_t h = 1; h <= 8192; h++) {
        const uint32_t per = (h + 3) / 4;
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t lo = k * per, hi = lo + per < h ? lo + per : h;      // rows [lo, hi), none when lo >= hi
            const uint32_t b0 = nyxhip::glcm_row_bounds_even(h, k), b1 = nyxhip::glcm_row_bounds_even(h, k + 1);
            if (lo < hi ? (b0 != lo || b1 != hi) : (b0 != b1)) same = 0;
        }
    }
    printf("%s glcm_row_bounds_even: ceil(h / 4) rows a wave\n", same ? "ok  " : "FAIL");
    if (!same) g_bad++;
    printf("shares %u %u %u %u of %u\n", nyxhip::kGlcmRowShare[0], nyxhip::kGlcmRowShare[1], nyxhip::kGlcmRowShare[2], nyxhip::kGlcmRowShare[3], nyxhip::kGlcmRowShareSum);
    if (g_bad) { printf("%d FAILED\n", g_bad); return 1; }
    printf("ALL PASSED\n");
    return 0;
}
