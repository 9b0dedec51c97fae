// test_wsgroup_plan.cpp -- the host plan of nyxhip_wsgroup_slides (nyxus_amd/csrc/wsgroup_plan.h) as a stand-alone program: the band cut
// covers every row exactly once with whole rows and at most WS_BAND_PIXELS pixels a band (one row where a row is longer), the workspace
// holds every record, and the chunks under a budget cover every slide once.  Driven by tests/test_wsgroup_plan_cpu.py, plain and under
// the address / undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include "../../nyxus_amd/csrc/wsgroup_plan.h"

using namespace nyxhip;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_cut(uint32_t w, uint32_t h)
{
    const uint32_t r = ws_band_rows(w), b = ws_bands(w, h);
    CHECK(r >= 1, "w %u", w);
    CHECK((uint64_t)r * w <= WS_BAND_PIXELS || r == 1, "w %u rows %u", w, r);
    CHECK((uint64_t)(r + 1) * w > WS_BAND_PIXELS, "w %u rows %u: a band could hold one more row", w, r);
    CHECK(b >= 1 && (uint64_t)b * r >= h && (uint64_t)(b - 1) * r < h, "w %u h %u rows %u bands %u", w, h, r, b);
    // what the kernels do with it: rows [band * r, min(h, band * r + r)) -- contiguous, disjoint, all of them, none empty
    uint64_t rows = 0;
    for (uint32_t band = 0; band < b; band++) {
        const uint32_t y0 = band * r, y1 = y0 + r < h ? y0 + r : h;
        CHECK(y0 < y1 && y0 == rows, "w %u h %u band %u", w, h, band);
        rows += y1 - y0;
        CHECK((uint64_t)y1 * w < (1ull << 32), "w %u h %u: a pixel index beyond 32 bits", w, h);
    }
    CHECK(rows == h, "w %u h %u", w, h);
    CHECK(ws_workspace_bytes(w, h) >= 8ull * ((uint64_t)kWsWords * b + kWsCentreWords + kWsBinWords), "w %u h %u", w, h);
    CHECK(ws_workspace_bytes(w, h) % 8 == 0, "w %u h %u", w, h);
}

static void check_chunks(uint32_t w, uint32_t h, uint32_t eb, bool host, uint64_t n, uint64_t budget, uint64_t want_chunks, uint64_t want_last)
{
    const WsPlan p = ws_plan(w, h, eb, host, n, 211, budget);
    CHECK(p.ok == 1, "w %u h %u budget %llu: ok %d", w, h, (unsigned long long)budget, p.ok);
    if (p.ok != 1) return;
    CHECK(p.chunk >= 1 && p.chunk <= 65535 && p.chunk <= n, "chunk %llu", (unsigned long long)p.chunk);
    CHECK(p.chunk * p.per_slide <= budget, "chunk %llu x %llu > %llu", (unsigned long long)p.chunk, (unsigned long long)p.per_slide, (unsigned long long)budget);
    CHECK(p.n_chunks == (n + p.chunk - 1) / p.chunk, "n_chunks");
    const uint64_t last = n - (p.n_chunks - 1) * p.chunk;
    CHECK(last >= 1 && last <= p.chunk, "last %llu", (unsigned long long)last);
    if (want_chunks) CHECK(p.n_chunks == want_chunks && last == want_last, "n %llu budget %llu: %llu chunks, last %llu (want %llu, %llu)", (unsigned long long)n,
                           (unsigned long long)budget, (unsigned long long)p.n_chunks, (unsigned long long)last, (unsigned long long)want_chunks, (unsigned long long)want_last);
    CHECK(p.band_rows == ws_band_rows(w) && p.bands == ws_bands(w, h) && p.ws_bytes == ws_workspace_bytes(w, h), "plan fields");
}

int main()
{
    // ---- the band cut: the full grid of small shapes, the seams of the constant, the extreme sides
    uint64_t shapes = 0;
    for (uint32_t w = 1; w <= 300; w++)
        for (uint32_t h = 1; h <= 300; h++) { check_cut(w, h); shapes++; }
    const uint32_t sides[] = {1, 2, 127, 128, 129, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 65533, 65534};
    for (uint32_t w : sides)
        for (uint32_t h : sides) { check_cut(w, h); shapes++; }
    CHECK(ws_band_rows(WS_BAND_PIXELS) == 1 && ws_band_rows(WS_BAND_PIXELS + 1) == 1 && ws_band_rows(WS_BAND_PIXELS / 2) == 2, "seams");
    CHECK(ws_bands(65534, 65534) == 65534 && ws_bands(1, 65534) == 4, "extreme sides: %u %u", ws_bands(65534, 65534), ws_bands(1, 65534));
    CHECK(ws_bands(128, 128) == 1 && ws_bands(128, 129) == 2 && ws_bands(128, 261) == 3, "the golden cases' bands");
    printf("band cut checked on %llu shapes\n", (unsigned long long)shapes);
    // ---- refusals
    CHECK(ws_plan(0, 5, 1, true, 1, 211, 1ull << 30).ok == 0 && ws_plan(5, 0, 1, true, 1, 211, 1ull << 30).ok == 0, "side 0");
    CHECK(ws_plan(65535, 5, 1, true, 1, 211, 1ull << 30).ok == 0 && ws_plan(5, 65535, 1, false, 1, 211, 1ull << 30).ok == 0, "side 65535");
    CHECK(ws_plan(65534, 65534, 4, false, 1, 211, 1ull << 40).ok == 1, "side 65534");
    CHECK(ws_plan(64, 64, 2, true, 3, 211, 1000).ok == -1, "a slide beyond the budget");
    // ---- chunks: budgets that give 1 / 2 / a shorter last chunk, device and host slides
    for (int host = 0; host < 2; host++)
        for (uint32_t eb = 1; eb <= 4; eb *= 2) {
            const uint64_t per = ws_plan(64, 48, eb, host != 0, 1, 211, 1ull << 40).per_slide;
            check_chunks(64, 48, eb, host != 0, 3, per * 3, 1, 3);              // everything at once (three slides: no forced split)
            check_chunks(64, 48, eb, host != 0, 6, per * 3 + per / 2, 2, 3);    // two full chunks
            check_chunks(64, 48, eb, host != 0, 7, per * 3, 3, 1);              // a shorter last chunk
            check_chunks(64, 48, eb, host != 0, 5, per, 5, 1);                  // a slide a chunk
            for (uint64_t n = 1; n <= 40; n++)
                for (uint64_t k = 1; k <= 9; k++) check_chunks(64, 48, eb, host != 0, n, per * k + 7, 0, 0);
        }
    // host slides overlap copy and sweep: at least two chunks from four slides on, and copies of at most 512 MiB
    CHECK(ws_plan(64, 48, 1, true, 4, 211, 1ull << 40).n_chunks == 2 && ws_plan(64, 48, 1, false, 4, 211, 1ull << 40).n_chunks == 1, "overlap rule");
    CHECK(ws_plan(16384, 16384, 4, true, 3, 211, 1ull << 42).chunk == 1, "512 MiB copies");
    CHECK(ws_plan(1, 1, 1, false, 100000, 7, 1ull << 40).chunk == 65535, "the grid dimension");
    if (fails) { printf("%d FAILED\n", fails); return 1; }
    printf("ALL PASSED\n");
    return 0;
}
