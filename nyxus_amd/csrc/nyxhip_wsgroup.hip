// nyxhip_wsgroup.hip -- the whole-slide group entries of include/nyxhip.h: nyxhip_wsgroup_n_columns / _column_name and
// nyxhip_wsgroup_slides, the contract of nyxhip_imq_slides over the kernels of roi_wsgroup.hip.  The plan (band cut, workspace,
// slides per chunk) is wsgroup_plan.h.
#include "nyxhip_ctx.h"
#include "batch_stage.h"
#include "roi_wsgroup.h"
#include "radial_close.h"

using namespace nyxhip;

namespace {

constexpr uint32_t kWsAll = NYXHIP_WS_CONTOUR | NYXHIP_WS_SMOMS | NYXHIP_WS_IMOMS | NYXHIP_WS_RADIAL;
constexpr int kWsContourCols = 7;

bool ws_mask_ok(uint32_t m) { return m != 0 && (m & ~kWsAll) == 0; }

int ws_n_columns(uint32_t m)
{
    return ((m & NYXHIP_WS_CONTOUR) ? kWsContourCols : 0) + ((m & NYXHIP_WS_SMOMS) ? kMomCols : 0) + ((m & NYXHIP_WS_IMOMS) ? kMomCols : 0) +
           ((m & NYXHIP_WS_RADIAL) ? kRadialCols : 0);
}

size_t ws_want(size_t need) { return need + need / 8 + (1 << 16); }

// nt slides resident on the device -> nt rows at d_out (device, leading dimension ld), enqueued on st
int ws_slides_chunk(nyxhip_ctx* ctx, const void* d_inten, int dt, uint32_t W, uint32_t H, uint32_t nt, uint32_t ws_mask, double* d_out, size_t ld, hipStream_t st)
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    const size_t o_off = o; o = al(o + 8 * ((size_t)nt + 1));
    const size_t o_smin = o; o = al(o + 8 * (size_t)nt);
    const size_t o_smax = o; o = al(o + 8 * (size_t)nt);
    size_t o_u[5]; for (int i = 0; i < 5; i++) { o_u[i] = o; o = al(o + 4 * (size_t)nt); }
    const size_t o_part = o; o = al(o + 8 * (size_t)kWsWords * (size_t)ws_bands(W, H) * nt);
    const size_t o_cen = o; o = al(o + 8 * (size_t)kWsCentreWords * nt);
    const size_t o_bins = o; o = al(o + 8 * (size_t)kWsBinWords * nt);
    HIP_TRY(ctx, ctx->d_tile.reserve(o, st, ws_want(o)));
    char* const base = ctx->d_tile.as<char>();
    SlideRows R{(uint32_t*)(base + o_u[0]), (uint64_t*)(base + o_off), (uint32_t*)(base + o_u[1]), (uint32_t*)(base + o_u[2]),
                (uint32_t*)(base + o_u[3]), (uint32_t*)(base + o_u[4]), (double*)(base + o_smin), (double*)(base + o_smax)};
    // the slide's maximum is the intensity of the four corner points: the extrema pass of every slide entry, for the contour block alone
    if (ws_mask & NYXHIP_WS_CONTOUR)
        if (int rc = launch_slide_headers(d_inten, dt, W, H, nt, R, st))
            return fail(ctx, NYXHIP_ERR_HIP, std::string("slide extrema launch failed: ") + hipGetErrorString((hipError_t)rc));
    WsArgs a;
    memset(&a, 0, sizeof(a));
    a.img = d_inten; a.dt = dt; a.w = W; a.h = H; a.n_slides = nt; a.ws_mask = ws_mask; a.vmax = R.vmax;
    a.partials = (uint64_t*)(base + o_part); a.centre = (uint64_t*)(base + o_cen); a.bins = (uint64_t*)(base + o_bins);
    a.wedge_tab = radial_wedge_tab();
    a.out = d_out; a.ld = ld;
    a.col_contour = 0;
    a.col_smoms = ws_n_columns(ws_mask & NYXHIP_WS_CONTOUR);
    a.col_imoms = ws_n_columns(ws_mask & (NYXHIP_WS_CONTOUR | NYXHIP_WS_SMOMS));
    a.col_radial = ws_n_columns(ws_mask & (NYXHIP_WS_CONTOUR | NYXHIP_WS_SMOMS | NYXHIP_WS_IMOMS));
    if (int rc = launch_wsgroup(a, st))
        return fail(ctx, NYXHIP_ERR_HIP, std::string("whole-slide group kernels: launch failed: ") + hipGetErrorString((hipError_t)rc));
    return NYXHIP_OK;
}

} // namespace

extern "C" {

int nyxhip_wsgroup_n_columns(uint32_t ws_mask)
{
    return ws_mask_ok(ws_mask) ? ws_n_columns(ws_mask) : -1;
}

int nyxhip_wsgroup_column_name(uint32_t ws_mask, int col, char* buf, size_t buf_len)
{
    if (!buf || buf_len == 0 || !ws_mask_ok(ws_mask) || col < 0 || col >= ws_n_columns(ws_mask)) return NYXHIP_ERR_INVALID_ARG;
    if (ws_mask & NYXHIP_WS_CONTOUR) {
        if (col < kWsContourCols) return nyxhip_morph_column_name(NYXHIP_MORPH_CONTOUR, col, buf, buf_len);
        col -= kWsContourCols;
    }
    nyxhip_settings s;
    nyxhip_default_settings(&s);
    const uint32_t bit[3] = {NYXHIP_WS_SMOMS, NYXHIP_WS_IMOMS, NYXHIP_WS_RADIAL}, fam[3] = {NYXHIP_FAM_SMOMS, NYXHIP_FAM_IMOMS, NYXHIP_FAM_RADIAL};
    for (int k = 0; k < 3; k++) {
        if (!(ws_mask & bit[k])) continue;
        const int n = nyxhip_n_columns(fam[k], &s);
        if (col < n) return nyxhip_column_name(fam[k], &s, col, buf, buf_len);
        col -= n;
    }
    return NYXHIP_ERR_INVALID_ARG;
}

int nyxhip_wsgroup_slides(nyxhip_ctx* ctx, const nyxhip_tiles* t, uint32_t ws_mask, const nyxhip_settings* s, double* out_table, size_t out_ld)
{
    if (!t || !s || !out_table) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null slides / settings / out_table");
    if (t->label) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "whole-slide mode takes no label image: slides->label must be NULL");
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (!ws_mask_ok(ws_mask)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "whole-slide group mask is zero or has a bit above NYXHIP_WS_RADIAL");
    if (t->inten_dtype != NYXHIP_U8 && t->inten_dtype != NYXHIP_U16 && t->inten_dtype != NYXHIP_U32)
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "slide element type must be NYXHIP_U8 / U16 / U32");
    if (t->memory != NYXHIP_MEM_HOST && t->memory != NYXHIP_MEM_DEVICE) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad memory kind");
    if (t->n_tiles == 0) return NYXHIP_OK;
    if (t->width == 0 || t->height == 0 || t->width > kWsMaxSide || t->height > kWsMaxSide)
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "whole-slide mode takes slides of 1 to 65534 pixels a side (coordinates inside an ROI are 16-bit)");
    if (!t->inten) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null slide pointer");
    const int n_cols = ws_n_columns(ws_mask);
    if (out_ld < (size_t)n_cols) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream();
    const bool host = t->memory == NYXHIP_MEM_HOST;
    const uint32_t W = t->width, H = t->height;
    const size_t in_bytes = (size_t)W * H * (size_t)t->inten_dtype;
    // ---- chunks of slides whose images and workspace fit the budget (the rule of nyxhip_featurize_slides; wsgroup_plan.h)
    size_t budget = (size_t)t->max_device_bytes;
    if (budget == 0) {
        size_t fr = 0, tot = 0;
        HIP_TRY(ctx, hipMemGetInfo(&fr, &tot));
        const int sharers = std::max(1, g_ctx_on_device[ctx->device & 63].load());
        budget = (fr + ctx->d_tile.bytes + ctx->d_slot[0].bytes + ctx->d_slot[1].bytes) / 2 / (size_t)sharers;
    }
    const WsPlan plan = ws_plan(W, H, (uint32_t)t->inten_dtype, host, t->n_tiles, (uint32_t)n_cols, budget);
    if (plan.ok < 0)
        return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "one slide and its workspace (" + std::to_string(plan.per_slide >> 20) + " MiB) do not fit max_device_bytes");
    const uint64_t chunk = plan.chunk, n_chunks = plan.n_chunks;

    if (!host) {
        for (uint64_t t0 = 0; t0 < t->n_tiles; t0 += chunk) {
            const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, t->n_tiles - t0);
            if (int rc = ws_slides_chunk(ctx, (const char*)t->inten + (size_t)t0 * in_bytes, t->inten_dtype, W, H, nt, ws_mask, out_table + t0 * out_ld, out_ld, st))
                return rc;
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return check_status(ctx);
    }

    // ---- host slides: chunk c + 1 is copied through the pinned staging ring while chunk c is reduced
    if (int prc = ensure_copy_pipeline(ctx)) return prc;
    const size_t slot_need = (size_t)chunk * in_bytes + 512;
    for (int k = 0; k < (n_chunks > 1 ? 2 : 1); k++)
        HIP_TRY(ctx, ctx->d_slot[k].reserve(slot_need, st, ws_want(slot_need)));
    if (int grc = ensure_stage(ctx, (size_t)chunk * n_cols * 8 + 256)) return grc;
    auto upload = [&](uint64_t c) -> int {                                  // chunk c -> slot c & 1 on the copy stream
        const int k = (int)(c & 1);
        const uint64_t t0 = c * chunk;
        const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, t->n_tiles - t0);
        if (c >= 2) HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->slot_free[k], 0));
        HIP_TRY(ctx, staged_h2d(ctx, ctx->d_slot[k].p, (const char*)t->inten + (size_t)t0 * in_bytes, (size_t)nt * in_bytes, ctx->copy_stream));
        HIP_TRY(ctx, hipEventRecord(ctx->slot_ready[k], ctx->copy_stream));
        return NYXHIP_OK;
    };
    StreamDrain drain{ctx->copy_stream, st};
    if (int urc = upload(0)) return urc;
    for (uint64_t c = 0; c < n_chunks; c++) {
        const int k = (int)(c & 1);
        const uint64_t t0 = c * chunk;
        const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, t->n_tiles - t0);
        HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->slot_ready[k], 0));
        double* const d_out = ctx->d_stage.as<double>();
        if (int rc = ws_slides_chunk(ctx, ctx->d_slot[k].p, t->inten_dtype, W, H, nt, ws_mask, d_out, (size_t)n_cols, st)) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->slot_free[k], st));
        if (c + 1 < n_chunks)
            if (int urc = upload(c + 1)) return urc;                        // the next chunk's copy runs beside this chunk's kernels
        HIP_TRY(ctx, hipMemcpy2DAsync(out_table + t0 * out_ld, out_ld * sizeof(double), d_out, (size_t)n_cols * sizeof(double), (size_t)n_cols * sizeof(double), nt,
                                      hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));                             // the chunk's rows are on the host; d_stage is free for the next one
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
    return check_status(ctx);
}

} // extern "C"
