// nyxhip_api.hip -- the C ABI of include/nyxhip.h: context, staging, launch, errors.
//
// Host-side counterpart of reduce_trivial_rois_manual()
// (the reference's src/nyx/reduce_trivial_rois.cpp:772-795): instead of fanning a
// label vector out over std::async threads per feature family (parallel.h:23-42),
// one fused kernel launch covers every requested family for the whole ROI batch.
#include "nyxhip_ctx.h"
#include "batch_stage.h"

using namespace nyxhip;

namespace nyxhip {

thread_local std::string g_init_error;
std::atomic<int> g_ctx_on_device[64];

int fail(nyxhip_ctx* ctx, int code, const std::string& msg)
{
    if (ctx)
        ctx->err = msg;
    else
        g_init_error = msg;
    return code;
}

} // namespace nyxhip

extern "C" {

int nyxhip_abi_version(void) { return NYXHIP_ABI_VERSION; }

int nyxhip_init(int device, nyxhip_ctx** out_ctx)
{
    if (!out_ctx) return NYXHIP_ERR_INVALID_ARG;
    *out_ctx = nullptr;
    (void)knob::at_start();   // the per-process knobs are what the environment says now, at the first context (knobs.h)
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, NYXHIP_ERR_NO_DEVICE, "no HIP device available: the MI355X path has no CPU fallback");
    if (device < 0 || device >= n)
        return fail(nullptr, NYXHIP_ERR_INVALID_ARG, "device index out of range");
    nyxhip_ctx* ctx = new nyxhip_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess ||
        ctx->d_status.reserve(4 * sizeof(int), nullptr) != hipSuccess || hipMemset(ctx->d_status.p, 0, 4 * sizeof(int)) != hipSuccess) {
        delete ctx;
        return fail(nullptr, NYXHIP_ERR_HIP, "failed to create the device context");
    }
    if (knob::stamps()) { // diagnostic builds only; never set in production
        if (ctx->d_stamps.reserve(32 * sizeof(unsigned long long), nullptr) == hipSuccess)
            (void)hipMemset(ctx->d_stamps.p, 0, 32 * sizeof(unsigned long long));
    }
    g_ctx_on_device[device & 63].fetch_add(1);
    *out_ctx = ctx;
    return NYXHIP_OK;
}

void nyxhip_destroy(nyxhip_ctx* ctx)
{
    if (!ctx) return;
    g_ctx_on_device[ctx->device & 63].fetch_sub(1);
    (void)hipSetDevice(ctx->device);
    // the streams first: nothing is in flight when the buffers free themselves (delete ctx)
    if (ctx->own_stream) { (void)hipStreamSynchronize(ctx->own_stream); (void)hipStreamDestroy(ctx->own_stream); }
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    for (hipStream_t s : ctx->lane_stream)
        if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (auto& p : ctx->ev) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (hipEvent_t e : {ctx->slot_ready[0], ctx->slot_ready[1], ctx->slot_free[0], ctx->slot_free[1], ctx->lane_fork})
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->lane_done)
        if (e) (void)hipEventDestroy(e);
    clear_runs(ctx);
    if (ctx->d_stamps) {
        unsigned long long h[32];
        if (hipMemcpy(h, ctx->d_stamps.p, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) {
            unsigned long long tot = 0;
            for (int i = 0; i < 32; i++) tot += h[i];
            for (int i = 0; i < 32; i++)
                if (h[i]) fprintf(stderr, "[nyxhip stamp] phase %2d: %14llu cycles  %5.1f %%\n", i, h[i], 100.0 * (double)h[i] / (double)tot);
        }
    }
    delete ctx;
}

const char* nyxhip_last_error(const nyxhip_ctx* ctx) { return ctx ? ctx->err.c_str() : g_init_error.c_str(); }

int nyxhip_set_stream(nyxhip_ctx* ctx, void* hip_stream)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    ctx->user_stream = (hipStream_t)hip_stream;
    ctx->use_user_stream = true; // NULL is the legacy default stream, a valid choice
    return NYXHIP_OK;
}

int nyxhip_sync(nyxhip_ctx* ctx)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream()));
    return check_status(ctx);
}

int nyxhip_featurize_batch_async_at(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y,
                                    uint32_t mask, const nyxhip_settings* s, double* out, size_t ld)
{
    int rc = validate(ctx, b, mask, s, out, ld);
    if (rc) return rc;
    if ((origin_x == nullptr) != (origin_y == nullptr))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "origin_x and origin_y must both be given or both NULL");
    if (b->memory != NYXHIP_MEM_DEVICE)
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "the async form takes device-resident batches only");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->n_roi == 0) return NYXHIP_OK;
    // batch extrema: the caller's statement when given (all of max_px / max_bbox_area / max_bbox_side non-zero), else the size
    // classifier of launch_device_all derives them on the device
    const bool hinted = b->max_px != 0 && b->max_bbox_area != 0 && b->max_bbox_side != 0;
    OriginScope origins(ctx, origin_x, origin_y);
    return launch_device(ctx, b, mask, s, out, ld, b->max_px, b->max_bbox_area, b->max_inten_range, b->max_bbox_side, hinted);
}

int nyxhip_featurize_batch_async(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s,
                                 double* out, size_t ld)
{
    return nyxhip_featurize_batch_async_at(ctx, b, nullptr, nullptr, mask, s, out, ld);
}

int nyxhip_featurize_batch(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s,
                           double* out, size_t ld)
{
    return nyxhip_featurize_batch_at(ctx, b, nullptr, nullptr, mask, s, out, ld);
}

int nyxhip_featurize_batch_at(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y,
                              uint32_t mask, const nyxhip_settings* s, double* out, size_t ld)
{
    if (int rc = validate(ctx, b, mask, s, out, ld)) return rc;
    BatchSpec sp{kReadXY | kReadInten | kReadBox | kReadRange | kReadSlide, "batch has null array pointers", nyxhip_n_columns(mask, s)};
    sp.origin_x = origin_x; sp.origin_y = origin_y;
    if (int rc = batch_check(ctx, sp, b, s, out, ld)) return rc;
    return batch_run(ctx, sp, b, out, ld, [&](const StagedBatch& g) {
        // a host batch: exact extrema and the census of the smallest size class (launch_device_all picks lists or filtered launches by it).
        // A device batch: the caller's statement when complete, else the size classifier of launch_device_all derives the extrema
        if (g.host) { ctx->census_small = g.n_small; ctx->census_total = g.d.n_roi; ctx->census_pending = 0; }
        OriginScope origins(ctx, g.d_ox, g.d_oy);
        return launch_device(ctx, &g.d, mask, s, g.d_out, g.ld, g.max_px, g.max_area, g.max_range, g.max_side, g.hinted);
    });
}

int nyxhip_timing_enable(nyxhip_ctx* ctx, int on)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    ctx->timing = on < 0 ? 0 : on > 2 ? 2 : on;
    return NYXHIP_OK;
}

int nyxhip_timing_reset(nyxhip_ctx* ctx)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    ctx->ev_used = 0;
    return NYXHIP_OK;
}

int nyxhip_timing_get(nyxhip_ctx* ctx, double* avg_kernel_ms, uint64_t* n_launches)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double tot = 0;
    for (size_t i = 0; i < ctx->ev_used; i++) {
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev[i].second));
        float ms = 0;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[i].first, ctx->ev[i].second));
        tot += ms;
    }
    if (avg_kernel_ms) *avg_kernel_ms = ctx->ev_used ? tot / (double)ctx->ev_used : 0.0;
    if (n_launches) *n_launches = ctx->ev_used;
    return NYXHIP_OK;
}

int nyxhip_debug_roi_words(nyxhip_ctx* ctx, uint64_t n_roi, uint64_t* n_orders, uint64_t* n_flags)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream()));
    std::vector<uint32_t> h(n_roi);
    auto count = [&](const uint32_t* d, uint64_t* out) -> int {
        if (!out) return NYXHIP_OK;
        *out = 0;
        if (!d || n_roi == 0) return NYXHIP_OK;
        // (the table of the last call holds at least its n_roi entries; a larger n_roi is the caller's error)
        if ((size_t)((const char*)d - ctx->d_roi_words.as<char>()) + 4ull * n_roi > ctx->d_roi_words.bytes)
            return fail(ctx, NYXHIP_ERR_INVALID_ARG, "n_roi exceeds the per-ROI tables of the last call");
        HIP_TRY(ctx, hipMemcpy(h.data(), d, 4ull * n_roi, hipMemcpyDeviceToHost));
        for (uint32_t v : h) *out += v != 0;
        return NYXHIP_OK;
    };
    if (int rc = count(ctx->glcm_ng, n_orders)) return rc;
    return count(ctx->close_flag, n_flags);
}

int nyxhip_launch_report(nyxhip_ctx* ctx, char* buf, size_t buf_len)
{
    if (!ctx) return -NYXHIP_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    std::string js = "[";
    for (size_t i = 0; i < ctx->runs.size(); i++) {
        const ClassRun& r = ctx->runs[i];
        char ms[48] = "null";
        if (r.e0 && r.e1 && hipEventSynchronize(r.e1) == hipSuccess) {
            float t = 0;
            if (hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess) snprintf(ms, sizeof(ms), "%.6f", (double)t);
        }
        char lane_ms[48] = "null";                      // from the class's start on the main stream to the end of its workspace lane
        if (r.e0 && r.e2 && hipEventSynchronize(r.e2) == hipSuccess) {
            float t = 0;
            if (hipEventElapsedTime(&t, r.e0, r.e2) == hipSuccess) snprintf(lane_ms, sizeof(lane_ms), "%.6f", (double)t);
        }
        char one[448];
        snprintf(one, sizeof(one), "%s{\"class\": %d, \"size_class\": %d, \"wide_range\": %d, \"rois\": %u, \"max_px\": %u, \"max_bbox_area\": %u, "
                 "\"max_range\": %u, \"max_side\": %u, \"workspace\": %d, \"cooperative\": %d, \"ms\": %s, \"lane_ms\": %s}", i ? ", " : "", r.cls, r.cls < 0 ? -1 : r.cls / 2, r.cls < 0 ? -1 : r.cls & 1,
                 r.count, r.E.px, r.E.area, r.E.range, r.E.side, r.workspace, r.cooperative, ms, lane_ms);
        js += one;
    }
    js += "]";
    if (buf && buf_len) {
        const size_t n = std::min(js.size(), buf_len - 1);
        memcpy(buf, js.data(), n);
        buf[n] = 0;
    }
    return (int)js.size();
}

} // extern "C"
