// deferred_chunk of nyxus_amd/csrc/deferred_list.h: the chunk arithmetic of the deferred-list launches, on the host alone (no HIP,
// no library).  Prints one line per check and "ALL PASSED"; exit code 1 on the first failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../nyxus_amd/csrc/deferred_list.h"

using nyxhip::deferred_chunk;

static int g_bad = 0;

static void expect(const char* what, uint64_t got, uint64_t want)
{
    const bool ok = got == want;
    printf("%s %s: %llu (want %llu)\n", ok ? "ok  " : "FAIL", what, (unsigned long long)got, (unsigned long long)want);
    if (!ok) g_bad++;
}

// the loop of deferred_chunks: every index once, in order, the last chunk = what is left
static void walk(const char* what, uint64_t n, uint64_t stride, uint64_t budget)
{
    const uint64_t chunk = deferred_chunk(n, stride, budget);
    std::vector<unsigned char> seen(n, 0);
    bool ok = chunk >= 1 && chunk <= (n ? n : 1) && (chunk == 1 || chunk * stride <= budget);
    uint64_t launches = 0, last = 0;
    for (uint64_t o = 0; o < n && ok; o += chunk) {
        const uint64_t count = n - o < chunk ? n - o : chunk;
        ok = count >= 1 && count <= chunk && count * stride <= (budget > stride ? budget : stride);
        for (uint64_t i = o; i < o + count && ok; i++) { ok = i < n && !seen[i]; seen[i] = 1; }
        launches++; last = count;
    }
    for (uint64_t i = 0; i < n && ok; i++) ok = seen[i] == 1;
    if (ok && n) ok = launches == (n + chunk - 1) / chunk && last == n - (launches - 1) * chunk;
    printf("%s walk %s: n %llu chunk %llu launches %llu last %llu\n", ok ? "ok  " : "FAIL", what, (unsigned long long)n, (unsigned long long)chunk,
           (unsigned long long)launches, (unsigned long long)last);
    if (!ok) g_bad++;
}

int main()
{
    const uint64_t GiB = 1ull << 30;
    expect("n = 1", deferred_chunk(1, 4096, GiB), 1);
    expect("n = 1, budget below one stride", deferred_chunk(1, 2 * GiB, GiB), 1);
    expect("budget below one stride", deferred_chunk(1000, GiB + 1, GiB), 1);
    expect("budget one byte below two strides", deferred_chunk(1000, GiB / 2 + 1, GiB), 1);
    expect("budget an exact multiple of the stride", deferred_chunk(1000, GiB / 8, GiB), 8);
    expect("budget one byte short of the multiple", deferred_chunk(1000, GiB / 8, GiB - 1), 7);
    expect("n below budget / stride", deferred_chunk(7, GiB / 8, GiB), 7);
    expect("n at budget / stride", deferred_chunk(8, GiB / 8, GiB), 8);
    expect("n above budget / stride", deferred_chunk(9, GiB / 8, GiB), 8);
    expect("stride 2^40, n = 2^31 - 1, 4 GiB", deferred_chunk((1ull << 31) - 1, 1ull << 40, 4 * GiB), 1);
    expect("stride 2^40, n = 2^31 - 1, 2^42 B", deferred_chunk((1ull << 31) - 1, 1ull << 40, 1ull << 42), 4);
    expect("stride 1, n = 2^31", deferred_chunk(1ull << 31, 1, 4 * GiB), 1ull << 31);
    expect("stride 2^40, n = 2^31, the largest budget", deferred_chunk(1ull << 31, 1ull << 40, ~0ull), (1ull << 24) - 1);
    expect("stride 0 is reported, not divided by", deferred_chunk(5, 0, GiB), 0);
    expect("stride 0, n = 0", deferred_chunk(0, 0, 0), 0);
    expect("n = 0", deferred_chunk(0, 4096, GiB), 1);
    walk("one chunk", 17, 192000, GiB);
    walk("chunk 5, 17 ROIs", 17, 192000, 1 << 20);
    walk("chunk 2, 7 ROIs", 7, 466688, 1 << 20);
    walk("chunk 1", 5, 2 << 20, 1 << 20);
    walk("n a multiple of the chunk", 20, 192000, 1 << 20);
    walk("one ROI", 1, 192000, 1 << 20);
    walk("a thousand ROIs, chunk 3", 1000, 300000, 1 << 20);
    if (g_bad) { printf("%d FAILED\n", g_bad); return 1; }
    printf("ALL PASSED\n");
    return 0;
}
