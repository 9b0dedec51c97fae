// nyxhip_tiles.hip -- the fused tile path: label + intensity tiles to feature rows, host staging, sharded entry points.
#include <thread>
#include <system_error>
#include "nyxhip_ctx.h"

using namespace nyxhip;

extern "C" {

// ---- fused tile path -----------------------------------------------------------------------------------------------------
static size_t tile_want(size_t need) { return need + need / 8 + (1 << 16); }     // allocation for a workspace of the tile path that must grow

static uint32_t log2u(uint32_t v) { uint32_t k = 0; while ((1u << k) < v) k++; return k; }

// Per-tile table size to start with: one slot per 1024 pixels (a 1024 x 1024 tile: 1024 slots for ~200 ROIs); a tile
// with more labels than slots makes the scan raise the overflow flag and the chunk is rescanned with four times the slots.
static uint32_t first_tile_cap(uint64_t tile_px)
{
    uint64_t c = tile_px / 1024;
    if (c < 256) c = 256;
    if (c > (1u << 22)) c = 1u << 22;
    return pow2ceil((uint32_t)c);
}

// Device workspace of one chunk besides the staging slots and the clouds (which are sized after the scan).
static size_t chunk_table_bytes(uint32_t nt, uint32_t cap)
{
    const size_t ent = (size_t)nt * cap;
    // per slot: 8 table words + 10 + 10 row words (unsorted / sorted rows) + three 8-byte arrays (CSR offsets, slide min / max) -- the
    // carve-out of tiles_chunk, kept in step with it; per 1024 slots: block sums; per tile: row / pixel starts and given slide extrema
    return ent * (28 * 4 + 3 * 8) + (ent / 1024 + 2) * 12 + (size_t)nt * (12 + 16) + 24 * 256 + (1 << 16);
}

// One chunk of tiles resident on the device -> rows in d_lab / d_til / d_out (device).  *n_roi_out rows are produced; more than
// rows_cap -> nothing is written beyond rows_cap and the caller reports the shortage.  `red` says whose columns the rows are: label
// scan, ROI assembly and row order are the same piece of code for every reducer.
static int tiles_chunk(nyxhip_ctx* ctx, const void* d_inten, int dtI, const void* d_label, int dtL, uint32_t W, uint32_t H, uint32_t nt,
                       int slide_mode, const double* h_smin, const double* h_smax, const TileReducer& red, const nyxhip_settings* s,
                       uint64_t rows_cap, uint32_t* d_lab, uint32_t* d_til, uint32_t tile_base, double* d_out, size_t d_ld, uint32_t label_limit,
                       uint64_t* n_roi_out, hipStream_t st)
{
    const uint32_t family_mask = red.mask;                               // (read on the Families paths only)
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    uint32_t cap = ctx->tile_cap_hint ? ctx->tile_cap_hint : first_tile_cap((uint64_t)W * H);
    const uint64_t tile_px = (uint64_t)W * H;
    const uint32_t cap_max = pow2ceil((uint32_t)std::min<uint64_t>(2 * tile_px, 1u << 30));
    if (cap > cap_max) cap = cap_max;
    uint32_t meta[16];
    TileRows R;
    char* base = nullptr;
    for (;;) {
        const uint64_t ent = (uint64_t)nt * cap;
        if (ent > (1ull << 31)) return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "too many ROIs per tile for one chunk: lower max_device_bytes so that fewer tiles share a chunk");
        const uint64_t rc_rows = ent;                                    // every ROI occupies a slot: this many rows always suffice
        size_t o = 0;
        size_t o_h[8]; for (int i = 0; i < 8; i++) { o_h[i] = o; o = al(o + 4 * ent); }
        size_t o_u[10]; for (int i = 0; i < 10; i++) { o_u[i] = o; o = al(o + 4 * (rc_rows + 1)); }
        size_t o_r[10]; for (int i = 0; i < 10; i++) { o_r[i] = o; o = al(o + 4 * (rc_rows + 1)); }
        const size_t o_ro = o; o = al(o + 8 * (rc_rows + 2));
        const size_t o_smin = o; o = al(o + 8 * (rc_rows + 1));
        const size_t o_smax = o; o = al(o + 8 * (rc_rows + 1));
        const size_t o_meta = o; o = al(o + 64);
        const size_t n_blk = (size_t)((ent + 1023) / 1024);
        const size_t o_br = o; o = al(o + 4 * n_blk);
        const size_t o_bp = o; o = al(o + 8 * n_blk);
        const size_t o_trb = o; o = al(o + 4 * ((size_t)nt + 1));
        const size_t o_tpb = o; o = al(o + 8 * ((size_t)nt + 1));
        const size_t o_sin = o; o = al(o + 16 * (size_t)nt);
        HIP_TRY(ctx, ctx->d_tile.reserve(o, st, tile_want(o)));
        base = ctx->d_tile.as<char>();
        TileHash T{(uint32_t*)(base + o_h[0]), (uint32_t*)(base + o_h[1]), (uint32_t*)(base + o_h[2]), (uint32_t*)(base + o_h[3]),
                   (uint32_t*)(base + o_h[4]), (uint32_t*)(base + o_h[5]), (uint32_t*)(base + o_h[6]), (uint32_t*)(base + o_h[7]), cap, 32u - log2u(cap)};
        TileRows U{(uint32_t*)(base + o_u[0]), (uint32_t*)(base + o_u[1]), (uint32_t*)(base + o_u[2]), nullptr, (uint32_t*)(base + o_u[3]),
                   (uint32_t*)(base + o_u[4]), (uint32_t*)(base + o_u[5]), (uint32_t*)(base + o_u[6]), (uint32_t*)(base + o_u[7]), (uint32_t*)(base + o_u[8]),
                   nullptr, nullptr};
        R = TileRows{(uint32_t*)(base + o_r[0]), (uint32_t*)(base + o_r[1]), (uint32_t*)(base + o_r[2]), (uint64_t*)(base + o_ro), (uint32_t*)(base + o_r[3]),
                     (uint32_t*)(base + o_r[4]), (uint32_t*)(base + o_r[5]), (uint32_t*)(base + o_r[6]), (uint32_t*)(base + o_r[7]), (uint32_t*)(base + o_r[8]),
                     (double*)(base + o_smin), (double*)(base + o_smax)};
        uint32_t* d_meta = (uint32_t*)(base + o_meta);
        HIP_TRY(ctx, hipMemsetAsync(d_meta, 0, 64, st));
        const double* d_smin = nullptr; const double* d_smax = nullptr;
        if (slide_mode == NYXHIP_SLIDE_GIVEN) {
            HIP_TRY(ctx, hipMemcpyAsync(base + o_sin, h_smin, 8 * (size_t)nt, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(base + o_sin + 8 * (size_t)nt, h_smax, 8 * (size_t)nt, hipMemcpyHostToDevice, st));
            d_smin = (const double*)(base + o_sin); d_smax = d_smin + nt;
        }
        int rc = launch_tile_assembly_scan(d_inten, dtI, d_label, dtL, W, H, nt, T, U, R, (uint32_t)std::min<uint64_t>(rc_rows, 0xFFFFFFFFu), d_meta,
                                           (uint32_t*)(base + o_br), (unsigned long long*)(base + o_bp), (uint32_t*)(base + o_trb),
                                           (unsigned long long*)(base + o_tpb), st);
        if (rc == 0)
            rc = launch_tile_rank(U, (const uint32_t*)(base + o_trb), (const unsigned long long*)(base + o_tpb), R, (uint32_t)std::min<uint64_t>(rc_rows, 0xFFFFFFFFu),
                                  nt, cap, slide_mode, d_smin, d_smax, st);
        if (rc) return fail(ctx, NYXHIP_ERR_HIP, std::string("tile scan launch failed: ") + hipGetErrorString((hipError_t)rc));
        HIP_TRY(ctx, hipMemcpyAsync(meta, d_meta, sizeof(meta), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (meta[7] == 1) {                                  // a tile holds more labels than its table has slots
            if (cap >= cap_max) return fail(ctx, NYXHIP_ERR_HIP, "tile table overflow at the maximum table size");
            cap = cap * 4 > cap_max ? cap_max : cap * 4;
            continue;
        }
        break;
    }
    ctx->tile_cap_hint = cap;
    if (meta[7] == 2)
        return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "an ROI's bounding box is wider or taller than 65535 pixels (coordinates inside a box are 16-bit)");
    if (meta[8] > label_limit)
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "the label tile holds a value above max_label");
    const uint64_t n_roi = meta[0];
    *n_roi_out = n_roi;
    if (n_roi == 0 || n_roi > rows_cap) return NYXHIP_OK;
    const uint64_t npx = ((uint64_t)meta[2] << 32) | meta[1];
    // INTENSITY / GLCM alone, every ROI LDS-sized: the feature kernel reads the ROIs' windows of the tiles itself and no cloud is
    // materialised (8 B per ROI pixel written and read back otherwise).  Any other family, or ROIs beyond LDS: clouds.
    bool window = !knob::no_window() && red.kind == TileReducer::Families && (family_mask & ~(uint32_t)(NYXHIP_FAM_INTENSITY | NYXHIP_FAM_GLCM)) == 0;   // (no_window: A/B and tests)
    if (window) {
        LdsLayout Lt; std::string why_t;
        window = make_layout(family_mask, s, nyxhip_n_columns(family_mask, s), meta[3], meta[4], meta[5], Lt, why_t) == NYXHIP_OK;
    }
    size_t c = 0;
    const size_t o_cx = c; c = al(c + 2 * npx);
    const size_t o_cy = c; c = al(c + 2 * npx);
    const size_t o_cv = c; c = al(c + 4 * npx);
    nyxhip_batch b;
    memset(&b, 0, sizeof(b));
    b.n_roi = n_roi; b.roi_label = R.label; b.px_offset = R.px_offset;
    b.bbox_w = R.bbox_w; b.bbox_h = R.bbox_h; b.min_inten = R.vmin; b.max_inten = R.vmax;
    b.slide_min = R.slide_min; b.slide_max = R.slide_max;
    b.memory = NYXHIP_MEM_DEVICE;
    auto make_clouds = [&]() -> int {
        HIP_TRY(ctx, ctx->d_cloud.reserve(c, st, tile_want(c)));
        char* const cb = ctx->d_cloud.as<char>();
        const int rc = launch_tile_clouds(d_inten, dtI, d_label, dtL, W, H, R, (uint32_t)n_roi, (uint16_t*)(cb + o_cx), (uint16_t*)(cb + o_cy), (uint32_t*)(cb + o_cv), st);
        if (rc) return fail(ctx, NYXHIP_ERR_HIP, std::string("cloud kernel launch failed: ") + hipGetErrorString((hipError_t)rc));
        b.x = (const uint16_t*)(cb + o_cx); b.y = (const uint16_t*)(cb + o_cy); b.inten = (const uint32_t*)(cb + o_cv);
        return NYXHIP_OK;
    };
    if (!window)
        if (int crc = make_clouds()) return crc;
    HIP_TRY(ctx, hipMemcpyAsync(d_lab, R.label, 4 * n_roi, hipMemcpyDeviceToDevice, st));
    if (d_til) {
        if (tile_base == 0) HIP_TRY(ctx, hipMemcpyAsync(d_til, R.tile, 4 * n_roi, hipMemcpyDeviceToDevice, st));
        else if (int arc = launch_add_offset(R.tile, tile_base, (uint32_t)n_roi, d_til, st))
            return fail(ctx, NYXHIP_ERR_HIP, std::string("tile index launch failed: ") + hipGetErrorString((hipError_t)arc));
    }
    if (window)
    {
        ctx->win_next = WindowSrc{d_inten, d_label, dtI, dtL, W, H, R.tile, R.label, R.bbox_x0, R.bbox_y0, knob::no_xcd_swizzle() ? 0u : 1u};   // (A/B knob)
    }
    // the box origins inside the tile: one tile is one image, so they are the reference's coordinates (the caliper classes read them);
    // the image-relating classes take the tile index as the image of a row
    switch (red.kind) {
    case TileReducer::Ih: return ih_device(ctx, &b, s, d_out, d_ld, meta[3]);
    case TileReducer::Imq: return imq_device(ctx, &b, s, d_out, d_ld, meta[4]);
    case TileReducer::Morph: return morph_device(ctx, &b, R.bbox_x0, R.bbox_y0, red.mask, s, d_out, d_ld, meta[3], meta[4], meta[6]);
    case TileReducer::Hexpoly:
        return hexpoly_device(ctx, &b, R.bbox_x0, R.bbox_y0, nullptr, 0, R.tile, red.pixel_distance, s, d_out, d_ld, meta[3], meta[4], meta[6]);
    case TileReducer::Neighbors:
        return neighbors_device(ctx, &b, R.bbox_x0, R.bbox_y0, nullptr, 0, R.tile, red.pixel_distance, s, d_out, d_ld, meta[3], meta[4], meta[6]);
    case TileReducer::Families: break;
    }
    OriginScope origins(ctx, R.bbox_x0, R.bbox_y0);
    int lrc = launch_device(ctx, &b, family_mask, s, d_out, d_ld, meta[3], meta[4], meta[5], meta[6]);
    ctx->win_next = WindowSrc{};
    if (lrc == NYXHIP_INTERNAL_NEEDS_CLOUDS) {
        // a size class of this chunk does not run from LDS under these settings (the whole-chunk extrema above could not tell: classes
        // get layouts of their own -- IBSI matrix orders, radix sort buffers of the wide-range classes): the workspace paths read clouds
        if (int crc = make_clouds()) return crc;
        lrc = launch_device(ctx, &b, family_mask, s, d_out, d_ld, meta[3], meta[4], meta[5], meta[6]);
    }
    return lrc;
}

// The column count of a reducer's rows.
static int reducer_n_cols(const TileReducer& red, const nyxhip_settings* s)
{
    switch (red.kind) {
    case TileReducer::Neighbors: return kNeighborCols;
    case TileReducer::Ih: return kIhCols;
    case TileReducer::Imq: return kImqCols;
    case TileReducer::Morph: return morph_n_columns(red.mask);
    case TileReducer::Hexpoly: return kHexpolyCols;
    case TileReducer::Families: break;
    }
    return nyxhip_n_columns(red.mask, s);
}

static int tiles_validate(nyxhip_ctx* ctx, const nyxhip_tiles* t, const TileReducer& red, const nyxhip_settings* s, uint64_t* n_roi_out)
{
    // (a class with entries of its own has checked its mask or distance there, and no family's settings are read for it)
    const bool families = red.kind == TileReducer::Families;
    const uint32_t family_mask = families ? red.mask : 0u;
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (!t || !s || !n_roi_out) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null tiles / settings / n_roi_out");
    if (t->n_tiles == 0) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "n_tiles must be >= 1");
    if (!t->inten || !t->label || t->width == 0 || t->height == 0) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null pointer or empty tile");
    auto dt_ok = [](int d) { return d == NYXHIP_U8 || d == NYXHIP_U16 || d == NYXHIP_U32; };
    if (!dt_ok(t->inten_dtype) || !dt_ok(t->label_dtype)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "tile element types must be NYXHIP_U8 / U16 / U32");
    if (families && (family_mask == 0 || (family_mask & ~kImplemented))) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad family mask");
    if (t->memory != NYXHIP_MEM_HOST && t->memory != NYXHIP_MEM_DEVICE && t->memory != NYXHIP_MEM_HOST_OWN_MAPPING) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad memory kind");
    if (t->slide_mode < NYXHIP_SLIDE_MONTAGE || t->slide_mode > NYXHIP_SLIDE_GIVEN) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad slide_mode");
    if (t->slide_mode == NYXHIP_SLIDE_GIVEN && (!t->slide_min || !t->slide_max)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "NYXHIP_SLIDE_GIVEN needs slide_min and slide_max");
    std::string why;
    if (!settings_ok(s, family_mask, why)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, why);
    return NYXHIP_OK;
}

// Room for `rows` result rows of n_cols columns in the context's device-resident result (rows already there are kept).
static int res_reserve(nyxhip_ctx* ctx, size_t rows, size_t n_cols, hipStream_t st)
{
    if (ctx->d_res && ctx->res_cols == n_cols && rows <= ctx->res_cap) return NYXHIP_OK;
    const bool carry = ctx->d_res && ctx->res_cols == n_cols && ctx->res_rows > 0;
    const size_t cap = std::max(rows, carry ? ctx->res_cap * 2 : (size_t)0);
    const size_t bytes = (((size_t)cap * n_cols * 8 + 255) & ~(size_t)255) + 8 * cap + 256;
    DevBuf nb;
    HIP_TRY(ctx, nb.reserve(bytes, nullptr));
    const double* o_tab = ctx->d_res ? ctx->res_table() : nullptr;
    const uint32_t* o_lab = ctx->d_res ? ctx->res_label() : nullptr;
    const uint32_t* o_til = ctx->d_res ? ctx->res_tile() : nullptr;
    const size_t o_rows = ctx->res_rows;
    DevBuf od = std::move(ctx->d_res);                 // (freed on every way out)
    ctx->d_res = std::move(nb); ctx->res_cap = cap; ctx->res_cols = n_cols;
    if (carry) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->res_table(), o_tab, o_rows * n_cols * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->res_label(), o_lab, o_rows * 4, hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->res_tile(), o_til, o_rows * 4, hipMemcpyDeviceToDevice, st));
    } else
        ctx->res_rows = 0;
    if (od) { HIP_TRY(ctx, hipStreamSynchronize(st)); od.release(); }
    return NYXHIP_OK;
}

} // extern "C"

namespace nyxhip {

// [src, src + bytes) of pageable host memory -> device through the context's pinned ring: per piece of at most kStageSlotBytes, wait for
// the slot's previous DMA, copy the piece into the slot with a few host threads (one thread moves ~10 GB/s, the link takes 50), enqueue
// the DMA, go on with the next slot.  Host copy of piece i + 1 and DMA of piece i overlap.
static void parallel_copy(void* dst, const void* src, size_t n)
{
    static const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned nt = (unsigned)std::min<size_t>(std::min(8u, std::max(1u, hw / 2)), n >> 21);     // >= 2 MiB per thread
    if (nt <= 1) { memcpy(dst, src, n); return; }
    std::vector<std::thread> th;
    const size_t per = ((n / nt) + 4095) & ~(size_t)4095;
    size_t rest = n;                                     // a thread could not be started: from its share on, the calling thread copies
    for (unsigned t = 1; t < nt; t++) {
        const size_t o = (size_t)t * per;
        if (o >= n) break;
        try { th.emplace_back([=]() { memcpy((char*)dst + o, (const char*)src + o, std::min(per, n - o)); }); }
        catch (const std::system_error&) { rest = o; break; }
    }
    memcpy(dst, src, std::min(per, n));
    if (rest < n) memcpy((char*)dst + rest, (const char*)src + rest, n - rest);
    for (auto& t : th) t.join();
}
hipError_t staged_h2d(nyxhip_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t st)
{
    // (no_staging: A/B knob, the runtime's own pageable path)
    if (knob::no_staging() || bytes < ((size_t)1 << 20)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    for (size_t o = 0; o < bytes; o += nyxhip_ctx::kStageSlotBytes) {
        const size_t len = std::min(nyxhip_ctx::kStageSlotBytes, bytes - o);
        const int k = ctx->h_stage_next;
        ctx->h_stage_next = (k + 1) % nyxhip_ctx::kStageSlots;
        PinnedSlot& slot = ctx->h_stage[k];
        if (hipError_t e = slot.ensure(nyxhip_ctx::kStageSlotBytes); e != hipSuccess) return e;
        if (slot.used)
            if (hipError_t e = hipEventSynchronize(slot.done); e != hipSuccess) return e;      // the slot's previous piece has left it
        parallel_copy(slot.p, (const char*)src + o, len);
        if (hipError_t e = hipMemcpyAsync((char*)dst + o, slot.p, len, hipMemcpyHostToDevice, st); e != hipSuccess) return e;
        if (hipError_t e = hipEventRecord(slot.done, st); e != hipSuccess) return e;
        slot.used = true;
    }
    return hipSuccess;
}

// The copy stream and the slot events of the host pipelines (tile path, whole-slide path): chunk c + 1 is copied into device slot (c + 1) & 1
// on the copy stream while the kernels of chunk c read slot c & 1 on the call's stream.
int ensure_copy_pipeline(nyxhip_ctx* ctx)
{
    if (ctx->copy_stream) return NYXHIP_OK;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (int k = 0; k < 2; k++) {
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->slot_ready[k], hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->slot_free[k], hipEventDisableTiming));
    }
    return NYXHIP_OK;
}

} // namespace nyxhip

extern "C" {

// Host tiles reach the device in one of two ways (nyxhip_tiles::memory):
//   NYXHIP_MEM_HOST              any host memory.  The bytes go through the library's OWN pinned staging ring (staged_h2d: hipHostMalloc'ed
//                                slots; a few host threads copy a piece into a slot, the DMA engine takes it from there, the next piece is
//                                copied meanwhile).  Nothing is assumed about the caller's allocator.
//   NYXHIP_MEM_HOST_OWN_MAPPING  the caller states that both arrays are mappings of their own (mmap, a page-aligned allocation that is not
//                                handed back to an allocator's arena while the call runs): their whole pages are registered for the call
//                                (hipHostRegister) and copied by DMA in place -- no staging copy.
// Round 3-5 registered whatever looked like a mapping of its own in /proc/self/maps (a rule that knew glibc's malloc only): pages of a
// malloc arena, registered and released, left the driver's user-pointer bookkeeping in a state in which a LATER copy from those
// addresses faulted on the GPU.  The decision now lies with the one who knows -- the caller.
// Only WHOLE PAGES inside the array are registered (rounded inward to 4 KiB; what lies in front of and behind them travels through the
// staging ring): two arrays of a call that share a page never overlap in a registration.  One guard per ARRAY: the sharded entry pins
// the whole stack once, before its threads copy their shares.
struct HostPin {
    void* p[2] = {nullptr, nullptr};
    uintptr_t lo[2] = {0, 0}, hi[2] = {0, 0};          // registered byte range of array k (empty: lo == hi)
    static constexpr uintptr_t kPage = 4096;
    void pin(int k, const void* ptr, size_t bytes)
    {
        if (knob::no_pin() || !ptr) return;   // (A/B knob)
        const uintptr_t a = ((uintptr_t)ptr + kPage - 1) & ~(kPage - 1), z = ((uintptr_t)ptr + bytes) & ~(kPage - 1);
        if (z <= a) return;                                   // no whole page inside the array
        if (hipHostRegister((void*)a, z - a, hipHostRegisterDefault) == hipSuccess) { p[k] = (void*)a; lo[k] = a; hi[k] = z; } else (void)hipGetLastError();
    }
    // host -> device copy of [src, src + bytes) of array k: the part inside the registered pages as one (DMA) copy, what lies in
    // front of and behind them as pageable copies
    hipError_t h2d(nyxhip_ctx* ctx, int k, void* dst, const void* src, size_t bytes, hipStream_t st) const
    {
        const uintptr_t b0 = (uintptr_t)src, b1 = b0 + bytes;
        const uintptr_t m0 = std::min(std::max(b0, lo[k]), b1), m1 = std::max(std::min(b1, hi[k]), m0);   // the registered middle [m0, m1)
        if (lo[k] == hi[k] || m0 == m1) return staged_h2d(ctx, dst, src, bytes, st);
        hipError_t e = hipSuccess;
        if (m0 > b0) e = staged_h2d(ctx, dst, src, m0 - b0, st);
        if (e == hipSuccess) e = hipMemcpyAsync((char*)dst + (m0 - b0), (const void*)m0, m1 - m0, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && b1 > m1) e = staged_h2d(ctx, (char*)dst + (m1 - b0), (const void*)m1, b1 - m1, st);
        return e;
    }
    ~HostPin()
    {
        for (void* q : p)
            if (q && hipHostUnregister(q) != hipSuccess) {
                (void)hipGetLastError();
                if (knob::debug()) fprintf(stderr, "[nyxhip] hipHostUnregister(%p) failed\n", q);
            }
    }
};

// The whole stack in chunks.  label_limit: v1's max_label (validated only).  prepinned: the caller has pinned the arrays.
static int tiles_run(nyxhip_ctx* ctx, const nyxhip_tiles* t, const TileReducer& red, const nyxhip_settings* s, uint32_t* out_labels, uint32_t* out_tile_index,
                     uint64_t max_rows, double* out_table, size_t out_ld, uint64_t* n_roi_out, uint32_t label_limit, uint32_t tile_index_base,
                     const HostPin* prepinned)
{
    if (int vrc = tiles_validate(ctx, t, red, s, n_roi_out)) return vrc;
    const int n_cols = reducer_n_cols(red, s);
    const bool host = t->memory == NYXHIP_MEM_HOST || t->memory == NYXHIP_MEM_HOST_OWN_MAPPING;
    const bool keep = host && out_table == nullptr;                  // result stays in the context (nyxhip_fetch_result)
    if (!keep && (!out_labels || !out_table)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null output pointers");
    if (!keep && (int)out_ld < n_cols) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *n_roi_out = 0;
    hipStream_t st = ctx->stream();
    const uint32_t W = t->width, H = t->height;
    const uint64_t tile_px = (uint64_t)W * H;
    const size_t tile_in_bytes = (size_t)tile_px * (size_t)(t->inten_dtype + t->label_dtype);
    // ---- chunking (the reference batches ROIs by ram_limit, phase2_2d.cpp:694-705): per tile the scan tables and rows, the
    // clouds (<= 8 B per pixel), the table rows and -- host input -- two staging copies of the tile
    size_t budget = (size_t)t->max_device_bytes;
    if (budget == 0) {
        size_t fr = 0, tot = 0;
        HIP_TRY(ctx, hipMemGetInfo(&fr, &tot));
        // half of what is free, shared with the other contexts living on this device (gpu_devices=[0, 0], two sharded contexts
        // on one GPU: each taking half of the free memory for itself would together claim all of it)
        const int sharers = std::max(1, g_ctx_on_device[ctx->device & 63].load());
        budget = (fr + ctx->d_tile.bytes + ctx->d_cloud.bytes + ctx->d_slot[0].bytes + ctx->d_slot[1].bytes) / 2 / (size_t)sharers;
    }
    const uint32_t cap0 = ctx->tile_cap_hint ? ctx->tile_cap_hint : first_tile_cap(tile_px);
    const size_t per_tile = chunk_table_bytes(1, cap0) + 8 * (size_t)tile_px + (size_t)cap0 * 8 * n_cols / 8 + (host ? 2 * tile_in_bytes : 0);
    uint64_t chunk = std::max<uint64_t>(1, budget / std::max<size_t>(per_tile, 1));
    if (host) chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(1, ((size_t)512 << 20) / tile_in_bytes));   // <= 512 MiB per copy: the pipeline needs chunks
    if (chunk > t->n_tiles) chunk = t->n_tiles;
    if (host && t->n_tiles >= 4 && chunk > (t->n_tiles + 1) / 2) chunk = (t->n_tiles + 1) / 2;                 // at least two chunks to overlap
    while ((uint64_t)chunk * cap0 > (1ull << 30) && chunk > 1) chunk /= 2;
    if (chunk > 65535) chunk = 65535;                      // the scan kernel spends grid.z on the tiles of a chunk (HIP: z <= 65535)
    // the per-tile table may grow while the stack is processed (a tile with more labels than slots: x 4 and rescan); the chunks
    // after that are sized for the table that is then in force
    auto rechunk = [&](uint64_t cur) -> uint64_t {
        const uint32_t capn = ctx->tile_cap_hint ? ctx->tile_cap_hint : cap0;
        if (capn <= cap0) return cur;
        const size_t pt = chunk_table_bytes(1, capn) + 8 * (size_t)tile_px + (size_t)capn * 8 * n_cols / 8 + (host ? 2 * tile_in_bytes : 0);
        uint64_t c2 = std::max<uint64_t>(1, budget / std::max<size_t>(pt, 1));
        while ((uint64_t)c2 * capn > (1ull << 30) && c2 > 1) c2 /= 2;
        return std::min(cur, c2);
    };

    if (keep) ctx->res_rows = 0;
    uint64_t rows_done = 0;
    bool short_out = false;
    if (!host) {
        for (uint64_t t0 = 0; t0 < t->n_tiles; t0 += chunk) {
            chunk = rechunk(chunk);
            const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, t->n_tiles - t0);
            const char* di = (const char*)t->inten + (size_t)t0 * tile_px * t->inten_dtype;
            const char* dl = (const char*)t->label + (size_t)t0 * tile_px * t->label_dtype;
            const uint64_t room = rows_done < max_rows ? max_rows - rows_done : 0;
            uint64_t n = 0;
            int rc = tiles_chunk(ctx, di, t->inten_dtype, dl, t->label_dtype, W, H, nt, t->slide_mode, t->slide_min ? t->slide_min + t0 : nullptr,
                                 t->slide_max ? t->slide_max + t0 : nullptr, red, s, short_out ? 0 : room, out_labels + rows_done,
                                 out_tile_index ? out_tile_index + rows_done : nullptr, (uint32_t)t0, out_table + rows_done * out_ld, out_ld, label_limit, &n, st);
            if (rc) return rc;
            if (n > room) short_out = true;
            rows_done += n;
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        *n_roi_out = rows_done;
        if (short_out) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "max_rows is smaller than the number of ROIs in the stack (see *n_roi_out)");
        return check_status(ctx);
    }

    // ---- host tiles: copy chunk c + 1 while chunk c is reduced --------------------------------------------------------------
    if (int prc = ensure_copy_pipeline(ctx)) return prc;
    const size_t slot_need = (size_t)chunk * tile_in_bytes + 512;
    const uint64_t n_chunks = (t->n_tiles + chunk - 1) / chunk;
    for (int k = 0; k < (n_chunks > 1 ? 2 : 1); k++)
        HIP_TRY(ctx, ctx->d_slot[k].reserve(slot_need, st, tile_want(slot_need)));
    auto slot_inten = [&](int k) { return ctx->d_slot[k].as<char>(); };
    auto slot_label = [&](int k, uint32_t nt) { return ctx->d_slot[k].as<char>() + (((size_t)nt * tile_px * t->inten_dtype + 255) & ~(size_t)255); };
    HostPin pin;                                        // (see HostPin: only on the caller's statement, unless the sharded entry pinned the stack)
    if (!prepinned && t->memory == NYXHIP_MEM_HOST_OWN_MAPPING) {
        pin.pin(0, t->inten, (size_t)t->n_tiles * tile_px * t->inten_dtype);
        pin.pin(1, t->label, (size_t)t->n_tiles * tile_px * t->label_dtype);
    }
    const HostPin* const pins = prepinned ? prepinned : &pin;
    auto upload = [&](uint64_t c) -> int {                                  // chunk c -> slot c & 1 on the copy stream
        const int k = (int)(c & 1);
        const uint64_t t0 = c * chunk;
        const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, t->n_tiles - t0);
        if (c >= 2) HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->slot_free[k], 0));      // the kernels of chunk c - 2 have let go of the slot
        HIP_TRY(ctx, pins->h2d(ctx, 0, slot_inten(k), (const char*)t->inten + (size_t)t0 * tile_px * t->inten_dtype, (size_t)nt * tile_px * t->inten_dtype, ctx->copy_stream));
        HIP_TRY(ctx, pins->h2d(ctx, 1, slot_label(k, nt), (const char*)t->label + (size_t)t0 * tile_px * t->label_dtype, (size_t)nt * tile_px * t->label_dtype, ctx->copy_stream));
        HIP_TRY(ctx, hipEventRecord(ctx->slot_ready[k], ctx->copy_stream));
        return NYXHIP_OK;
    };
    // every exit below -- the error returns included -- first waits for the copies and kernels still in flight: the pin guard above
    // unregisters the caller's arrays, and the caller may free them the moment this function returns
    StreamDrain drain{ctx->copy_stream, st};
    if (int urc = upload(0)) return urc;
    for (uint64_t c = 0; c < n_chunks; c++) {
        const int k = (int)(c & 1);
        const uint64_t t0 = c * chunk;
        const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, t->n_tiles - t0);
        HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->slot_ready[k], 0));
        uint64_t n = 0;
        // the chunk's rows are produced in a device block owned by the context (d_stage), then copied out.  Its size follows the
        // ROI density seen so far (first chunk: 256 per tile); a denser chunk is rescanned once with the room it asked for.
        const uint64_t est_rows = std::max<uint64_t>((uint64_t)nt * 256, t0 ? (rows_done * 5 / 4 / t0 + 1) * nt : 0);
        size_t need = (size_t)est_rows * (8 * (size_t)n_cols + 8) + 1024;
        int rc;
        for (;;) {
            uint64_t cap_rows;
            double* d_out; uint32_t *d_lab, *d_til;
            if (keep) {                                   // rows are appended to the context's device-resident result: no copy, no sync per chunk
                if (int grc = res_reserve(ctx, (size_t)(rows_done + std::max<uint64_t>(est_rows, n)), (size_t)n_cols, st)) return grc;
                cap_rows = ctx->res_cap - rows_done;
                d_out = ctx->res_table() + rows_done * (size_t)n_cols; d_lab = ctx->res_label() + rows_done; d_til = ctx->res_tile() + rows_done;
            } else {
                if (int grc = ensure_stage(ctx, need)) return grc;
                cap_rows = (ctx->d_stage.bytes - 1024) / (8 * (size_t)n_cols + 8);
                d_out = ctx->d_stage.as<double>();
                d_lab = (uint32_t*)(ctx->d_stage.as<char>() + (((size_t)cap_rows * 8 * n_cols + 255) & ~(size_t)255));
                d_til = d_lab + cap_rows;
            }
            rc = tiles_chunk(ctx, slot_inten(k), t->inten_dtype, slot_label(k, nt), t->label_dtype, W, H, nt, t->slide_mode,
                             t->slide_min ? t->slide_min + t0 : nullptr, t->slide_max ? t->slide_max + t0 : nullptr, red, s, cap_rows, d_lab, d_til,
                             tile_index_base + (uint32_t)t0, d_out, (size_t)n_cols, label_limit, &n, st);
            if (rc) return rc;
            if (n > cap_rows) { HIP_TRY(ctx, hipStreamSynchronize(st)); need = (size_t)n * (8 * (size_t)n_cols + 8) + 4096; continue; }
            HIP_TRY(ctx, hipEventRecord(ctx->slot_free[k], st));
            if (c + 1 < n_chunks)
                if (int urc = upload(c + 1)) return urc;                    // the next chunk's DMA runs beside this chunk's kernels
            const uint64_t room = rows_done < max_rows ? max_rows - rows_done : 0;
            if (keep) {
                ctx->res_rows = (size_t)(rows_done + n);
            } else if (n <= room && !short_out) {
                if (n) {
                    HIP_TRY(ctx, hipMemcpy2DAsync(out_table + rows_done * out_ld, out_ld * sizeof(double), d_out, (size_t)n_cols * sizeof(double),
                                                  (size_t)n_cols * sizeof(double), n, hipMemcpyDeviceToHost, st));
                    HIP_TRY(ctx, hipMemcpyAsync(out_labels + rows_done, d_lab, 4 * n, hipMemcpyDeviceToHost, st));
                    if (out_tile_index) HIP_TRY(ctx, hipMemcpyAsync(out_tile_index + rows_done, d_til, 4 * n, hipMemcpyDeviceToHost, st));
                }
                HIP_TRY(ctx, hipStreamSynchronize(st));                     // the chunk's rows are on the host; d_stage is free for the next one
            } else {
                short_out = true;
                HIP_TRY(ctx, hipStreamSynchronize(st));
            }
            break;
        }
        rows_done += n;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *n_roi_out = rows_done;
    if (short_out) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "max_rows is smaller than the number of ROIs in the stack (see *n_roi_out)");
    return check_status(ctx);
}

int nyxhip_featurize_tiles_v2(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, uint32_t family_mask, const nyxhip_settings* s, uint32_t* out_labels,
                              uint32_t* out_tile_index, uint64_t max_rows, double* out_table, size_t out_ld, uint64_t* n_roi_out)
{
    return tiles_run(ctx, tiles, {TileReducer::Families, family_mask, 0}, s, out_labels, out_tile_index, max_rows, out_table, out_ld, n_roi_out, 0xFFFFFFFFu, 0, nullptr);
}

int nyxhip_neighbors_tiles(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, int32_t pixel_distance, const nyxhip_settings* s, uint32_t* out_labels,
                           uint32_t* out_tile_index, uint64_t max_rows, double* out_table, size_t out_ld, uint64_t* n_roi_out)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (int rc = pixel_distance_check(ctx, pixel_distance)) return rc;
    return tiles_run(ctx, tiles, {TileReducer::Neighbors, 0, pixel_distance}, s, out_labels, out_tile_index, max_rows, out_table, out_ld, n_roi_out, 0xFFFFFFFFu, 0, nullptr);
}

int nyxhip_ih_tiles(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, const nyxhip_settings* s, uint32_t* out_labels, uint32_t* out_tile_index, uint64_t max_rows,
                    double* out_table, size_t out_ld, uint64_t* n_roi_out)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (!s) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null tiles / settings / n_roi_out");
    if (int rc = ih_settings_check(ctx, s)) return rc;
    return tiles_run(ctx, tiles, {TileReducer::Ih, 0, 0}, s, out_labels, out_tile_index, max_rows, out_table, out_ld, n_roi_out, 0xFFFFFFFFu, 0, nullptr);
}

int nyxhip_imq_tiles(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, const nyxhip_settings* s, uint32_t* out_labels, uint32_t* out_tile_index, uint64_t max_rows,
                     double* out_table, size_t out_ld, uint64_t* n_roi_out)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    const int rc = tiles_run(ctx, tiles, {TileReducer::Imq, 0, 0}, s, out_labels, out_tile_index, max_rows, out_table, out_ld, n_roi_out, 0xFFFFFFFFu, 0, nullptr);
    return rc == NYXHIP_ERR_UNSUPPORTED ? fail(ctx, rc, kImqWidthMessage) : rc;
}

int nyxhip_morph_tiles(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, uint32_t morph_mask, const nyxhip_settings* s, uint32_t* out_labels,
                       uint32_t* out_tile_index, uint64_t max_rows, double* out_table, size_t out_ld, uint64_t* n_roi_out)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (nyxhip_morph_n_columns(morph_mask) < 0) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad morphology mask");
    return tiles_run(ctx, tiles, {TileReducer::Morph, morph_mask, 0}, s, out_labels, out_tile_index, max_rows, out_table, out_ld, n_roi_out, 0xFFFFFFFFu, 0, nullptr);
}

int nyxhip_hexpoly_tiles(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, int32_t pixel_distance, const nyxhip_settings* s, uint32_t* out_labels,
                         uint32_t* out_tile_index, uint64_t max_rows, double* out_table, size_t out_ld, uint64_t* n_roi_out)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (int rc = pixel_distance_check(ctx, pixel_distance)) return rc;
    return tiles_run(ctx, tiles, {TileReducer::Hexpoly, 0, pixel_distance}, s, out_labels, out_tile_index, max_rows, out_table, out_ld, n_roi_out, 0xFFFFFFFFu, 0, nullptr);
}

int nyxhip_fetch_result(nyxhip_ctx* ctx, uint32_t* out_labels, uint32_t* out_tile_index, double* out_table, size_t out_ld)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    const size_t n = ctx->res_rows, nc = ctx->res_cols;
    if (n && (!out_labels || !out_table || out_ld < nc)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null output pointers or out_ld smaller than the column count");
    if (n) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream();
        HIP_TRY(ctx, hipMemcpy2DAsync(out_table, out_ld * sizeof(double), ctx->res_table(), nc * sizeof(double), nc * sizeof(double), n, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(out_labels, ctx->res_label(), 4 * n, hipMemcpyDeviceToHost, st));
        if (out_tile_index) HIP_TRY(ctx, hipMemcpyAsync(out_tile_index, ctx->res_tile(), 4 * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    ctx->res_rows = 0;                                 // (the device block is kept for the next call)
    return NYXHIP_OK;
}

int nyxhip_featurize_tiles_sharded(nyxhip_ctx* const* ctxs, int n_ctx, const nyxhip_tiles* tiles, uint32_t family_mask, const nyxhip_settings* s,
                                   uint32_t* out_labels, uint32_t* out_tile_index, uint64_t max_rows, double* out_table, size_t out_ld, uint64_t* n_roi_out)
{
    if (!ctxs || n_ctx < 1 || !ctxs[0]) return NYXHIP_ERR_INVALID_ARG;
    nyxhip_ctx* c0 = ctxs[0];
    if (!tiles || !n_roi_out) return fail(c0, NYXHIP_ERR_INVALID_ARG, "null tiles / n_roi_out");
    if (tiles->memory != NYXHIP_MEM_HOST && tiles->memory != NYXHIP_MEM_HOST_OWN_MAPPING) return fail(c0, NYXHIP_ERR_INVALID_ARG, "the sharded entry takes host-memory stacks (every context copies its own share)");
    const bool keep = out_table == nullptr;                              // results stay in the contexts (nyxhip_fetch_result_sharded)
    if (!keep && !out_labels) return fail(c0, NYXHIP_ERR_INVALID_ARG, "null output pointers");
    for (int g = 0; g < n_ctx; g++)
        if (!ctxs[g]) return fail(c0, NYXHIP_ERR_INVALID_ARG, "null context in the list");
    const int G = (int)std::min<uint64_t>((uint64_t)n_ctx, tiles->n_tiles ? tiles->n_tiles : 1);
    // contiguous block partition (the first n % G contexts get one tile more); every context keeps its rows, which are then
    // laid out back to back in context order = stack order
    std::vector<int> rcs(G, 0);
    std::vector<uint64_t> cnt(G, 0), lo(G + 1, 0);
    const uint64_t q = tiles->n_tiles / G, r = tiles->n_tiles % G;
    for (int g = 0; g < G; g++) lo[g + 1] = lo[g] + q + ((uint64_t)g < r ? 1 : 0);
    const uint64_t tile_px = (uint64_t)tiles->width * tiles->height;
    for (int g = 0; g < n_ctx; g++) ctxs[g]->res_rows = 0;
    HostPin pin;                                        // the whole stack, once: released after every share's copies have drained (join below)
    if (tiles->memory == NYXHIP_MEM_HOST_OWN_MAPPING && hipSetDevice(c0->device) == hipSuccess) {
        pin.pin(0, tiles->inten, (size_t)tiles->n_tiles * tile_px * tiles->inten_dtype);
        pin.pin(1, tiles->label, (size_t)tiles->n_tiles * tile_px * tiles->label_dtype);
    } else (void)hipGetLastError();
    std::vector<std::thread> th;
    for (int g = 0; g < G; g++)
        th.emplace_back([&, g]() {
            nyxhip_tiles part = *tiles;
            part.n_tiles = (uint32_t)(lo[g + 1] - lo[g]);
            part.inten = (const char*)tiles->inten + (size_t)lo[g] * tile_px * tiles->inten_dtype;
            part.label = (const char*)tiles->label + (size_t)lo[g] * tile_px * tiles->label_dtype;
            if (tiles->slide_min) part.slide_min = tiles->slide_min + lo[g];
            if (tiles->slide_max) part.slide_max = tiles->slide_max + lo[g];
            if (part.n_tiles == 0) { rcs[g] = 0; return; }
            rcs[g] = tiles_run(ctxs[g], &part, {TileReducer::Families, family_mask, 0}, s, nullptr, nullptr, 0, nullptr, 0, &cnt[g], 0xFFFFFFFFu, (uint32_t)lo[g], &pin);   // tile indices of the whole stack
        });
    for (auto& t : th) t.join();
    for (int g = 0; g < G; g++)
        if (rcs[g]) return g == 0 ? rcs[g] : fail(c0, rcs[g], std::string("context ") + std::to_string(g) + ": " + ctxs[g]->err);
    uint64_t total = 0;
    for (int g = 0; g < G; g++) total += cnt[g];
    *n_roi_out = total;
    if (keep) return NYXHIP_OK;
    if (total > max_rows) {
        for (int g = 0; g < G; g++) ctxs[g]->res_rows = 0;
        return fail(c0, NYXHIP_ERR_INVALID_ARG, "max_rows is smaller than the number of ROIs in the stack (see *n_roi_out)");
    }
    return nyxhip_fetch_result_sharded(ctxs, n_ctx, out_labels, out_tile_index, out_table, out_ld);
}

int nyxhip_fetch_result_sharded(nyxhip_ctx* const* ctxs, int n_ctx, uint32_t* out_labels, uint32_t* out_tile_index, double* out_table, size_t out_ld)
{
    if (!ctxs || n_ctx < 1) return NYXHIP_ERR_INVALID_ARG;
    uint64_t row = 0;
    for (int g = 0; g < n_ctx; g++) {
        if (!ctxs[g]) return NYXHIP_ERR_INVALID_ARG;
        const uint64_t n = ctxs[g]->res_rows;
        if (n) {
            int rc = nyxhip_fetch_result(ctxs[g], out_labels + row, out_tile_index ? out_tile_index + row : nullptr, out_table + row * out_ld, out_ld);
            if (rc) return rc;
        }
        row += n;
    }
    return NYXHIP_OK;
}

int nyxhip_featurize_tile(nyxhip_ctx* ctx, const uint32_t* inten, const uint32_t* label, uint32_t width, uint32_t height,
                          int32_t memory, uint32_t max_label, uint32_t family_mask, const nyxhip_settings* s,
                          uint32_t* out_labels, uint64_t max_rows, double* out_table, size_t out_ld, uint64_t* n_roi_out)
{
    return nyxhip_featurize_tiles(ctx, inten, label, width, height, 1, memory, max_label, family_mask, s, out_labels, nullptr,
                                  max_rows, out_table, out_ld, n_roi_out);
}

int nyxhip_featurize_tiles(nyxhip_ctx* ctx, const uint32_t* inten, const uint32_t* label, uint32_t width, uint32_t height,
                           uint32_t n_tiles, int32_t memory, uint32_t max_label, uint32_t family_mask, const nyxhip_settings* s,
                           uint32_t* out_labels, uint32_t* out_tile_index, uint64_t max_rows, double* out_table, size_t out_ld,
                           uint64_t* n_roi_out)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (!out_labels || !out_table) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null pointer or empty tile");
    nyxhip_tiles t;
    memset(&t, 0, sizeof(t));
    t.inten = inten; t.label = label; t.inten_dtype = NYXHIP_U32; t.label_dtype = NYXHIP_U32;
    t.width = width; t.height = height; t.n_tiles = n_tiles; t.memory = memory; t.slide_mode = NYXHIP_SLIDE_MONTAGE;
    return tiles_run(ctx, &t, {TileReducer::Families, family_mask, 0}, s, out_labels, out_tile_index, max_rows, out_table, out_ld, n_roi_out, max_label, 0, nullptr);
}

} // extern "C"
