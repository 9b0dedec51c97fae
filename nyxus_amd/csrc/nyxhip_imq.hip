// nyxhip_imq.hip -- the image-quality entries of include/nyxhip.h: column names, the launches over a device-resident batch (imq_device),
// nyxhip_imq_batch and nyxhip_imq_slides.  The tile entry (nyxhip_imq_tiles) lives with the tile path in nyxhip_tiles.hip.
#include "nyxhip_ctx.h"
#include "deferred_list.h"
#include "batch_stage.h"

using namespace nyxhip;

namespace nyxhip {

static const char* const kImqNames[kImqCols] = {"FOCUS_SCORE", "LOCAL_FOCUS_SCORE", "MAX_SATURATION", "MIN_SATURATION"};

const char* const kImqWidthMessage =
    "image quality: 4 * max_inten * bbox_w * bbox_h of an ROI reaches 2^63 (the 64-bit sum of the Laplacian could wrap)";

// check_status with this class's reading of NYXHIP_ERR_UNSUPPORTED (the kernels of roi_imq.hip raise it for the width bound alone)
int imq_check_status(nyxhip_ctx* ctx)
{
    const int rc = check_status(ctx);
    return rc == NYXHIP_ERR_UNSUPPORTED ? fail(ctx, rc, kImqWidthMessage) : rc;
}

int imq_device(nyxhip_ctx* ctx, const nyxhip_batch* b, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_area)
{
    if (b->n_roi == 0) return NYXHIP_OK;
    hipStream_t st = ctx->stream();
    ImqArgs a;
    memset(&a, 0, sizeof(a));
    a.n_roi = b->n_roi; a.px_offset = b->px_offset; a.x = b->x; a.y = b->y; a.inten = b->inten; a.bbox_w = b->bbox_w; a.bbox_h = b->bbox_h;
    a.vmin = b->min_inten; a.vmax = b->max_inten; a.soft_nan = s->soft_nan; a.out = d_out; a.ld = ld; a.status = ctx->d_status.as<int>();
    // max_area == 0: not known.  Every ROI belongs to exactly one form by its box; a form without a member is not launched when that
    // is known.  (An empty ROI belongs to the wave form, which writes its soft_nan row.)
    const bool block_form = max_area == 0 || max_area > kImqWaveCells, list_form = max_area == 0 || max_area > kImqLdsCells;
    if (int rc = launch_roi_imq(a, st, true, block_form, max_area ? max_area : kImqLdsCells))
        return fail(ctx, NYXHIP_ERR_HIP, std::string("image-quality kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
    if (!list_form) return NYXHIP_OK;
    // boxes beyond the LDS plane: classifier, one read-back, a list launch over global planes
    DeferredList listed;
    if (int rc = deferred_build(ctx, "image quality", ctx->d_imq.list, b->n_roi, ImqListed{b->px_offset, b->bbox_w, b->bbox_h, kImqLdsCells}, st, listed)) return rc;
    if (int rc = deferred_count(ctx, listed, st)) return rc;
    if (!listed.hdr[0]) return NYXHIP_OK;
    ImqArgs aw = a;
    aw.ws_stride = ((uint64_t)listed.hdr[1] + 63) & ~63ull;
    return deferred_chunks(ctx, "image quality", listed, 4 * aw.ws_stride, (size_t)1 << 30, ctx->d_imq.ws, st, [&](const uint32_t* list, uint32_t count) {
        aw.ws = ctx->d_imq.ws.as<uint32_t>(); aw.roi_index = list;
        return launch_roi_imq_list(aw, st, count) != 0 ? fail(ctx, NYXHIP_ERR_HIP, "image-quality kernel: launch failed") : NYXHIP_OK;
    });
}

} // namespace nyxhip

namespace {

constexpr uint32_t kSlideMaxSide = 65534;         // the batch ABI's coordinates are 16-bit (nyxhip_featurize_slides)

size_t imq_want(size_t need) { return need + need / 8 + (1 << 16); }

// nt slides resident on the device -> nt rows at d_out (device, leading dimension ld), enqueued on st
int imq_slides_chunk(nyxhip_ctx* ctx, const void* d_inten, int dt, uint32_t W, uint32_t H, uint32_t nt, const nyxhip_settings* s, double* d_out, size_t ld,
                     hipStream_t st)
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint64_t recs = imq_slide_records(W, H);
    size_t o = 0;
    const size_t o_off = o; o = al(o + 8 * ((size_t)nt + 1));
    const size_t o_smin = o; o = al(o + 8 * (size_t)nt);
    const size_t o_smax = o; o = al(o + 8 * (size_t)nt);
    size_t o_u[5]; for (int i = 0; i < 5; i++) { o_u[i] = o; o = al(o + 4 * (size_t)nt); }
    const size_t o_part = o; o = al(o + 8 * (size_t)kImqWords * (size_t)recs * nt);
    HIP_TRY(ctx, ctx->d_tile.reserve(o, st, imq_want(o)));
    char* const base = ctx->d_tile.as<char>();
    SlideRows R{(uint32_t*)(base + o_u[0]), (uint64_t*)(base + o_off), (uint32_t*)(base + o_u[1]), (uint32_t*)(base + o_u[2]),
                (uint32_t*)(base + o_u[3]), (uint32_t*)(base + o_u[4]), (double*)(base + o_smin), (double*)(base + o_smax)};
    // the slide's extrema: the pass the slide path makes for every family
    if (int rc = launch_slide_headers(d_inten, dt, W, H, nt, R, st))
        return fail(ctx, NYXHIP_ERR_HIP, std::string("slide extrema launch failed: ") + hipGetErrorString((hipError_t)rc));
    if (int rc = launch_imq_slides(d_inten, dt, W, H, nt, R.vmin, R.vmax, (uint64_t*)(base + o_part), s->soft_nan, d_out, ld, ctx->d_status.as<int>(), st))
        return fail(ctx, NYXHIP_ERR_HIP, std::string("image-quality slide kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
    return NYXHIP_OK;
}

} // namespace

extern "C" {

int nyxhip_imq_column_name(int col, char* buf, size_t buf_len)
{
    if (!buf || buf_len == 0 || col < 0 || col >= kImqCols) return NYXHIP_ERR_INVALID_ARG;
    snprintf(buf, buf_len, "%s", kImqNames[col]);
    return NYXHIP_OK;
}

int nyxhip_imq_batch(nyxhip_ctx* ctx, const nyxhip_batch* b, const nyxhip_settings* s, double* out, size_t ld)
{
    BatchSpec sp{kReadXY | kReadInten | kReadBox | kReadRange,
                 "batch has null array pointers (the image-quality entries read px_offset, x, y, inten, bbox_w, bbox_h, min_inten, max_inten)", kImqCols};
    sp.status = imq_check_status;
    if (int rc = batch_check(ctx, sp, b, s, out, ld)) return rc;
    // ROI r of a host batch: the box within 16-bit coordinates, and the width bound the kernels of roi_imq.hip raise on a device batch
    auto roi_check = [&](uint64_t r) {
        if (b->bbox_w[r] > 65535u || b->bbox_h[r] > 65535u) return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "an ROI's bounding box is wider or taller than 65535 pixels");
        const uint64_t cells = (uint64_t)b->bbox_w[r] * b->bbox_h[r];
        if (b->px_offset[r + 1] > b->px_offset[r] && cells && (uint64_t)b->max_inten[r] * cells >= (1ull << 61)) return fail(ctx, NYXHIP_ERR_UNSUPPORTED, kImqWidthMessage);
        return (int)NYXHIP_OK;
    };
    return batch_run(ctx, sp, b, out, ld, [&](const StagedBatch& g) {
        // the largest box: a host batch's at least 1 (known), a device batch's as stated beside max_px (0: not known)
        return imq_device(ctx, &g.d, s, g.d_out, g.ld, g.host ? std::max(g.max_area, 1u) : g.max_px ? g.max_area : 0u);
    }, roi_check);
}

int nyxhip_imq_slides(nyxhip_ctx* ctx, const nyxhip_tiles* t, const nyxhip_settings* s, double* out_table, size_t out_ld)
{
    if (!t || !s || !out_table) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null slides / settings / out_table");
    if (t->label) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "whole-slide mode takes no label image: slides->label must be NULL");
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (t->inten_dtype != NYXHIP_U8 && t->inten_dtype != NYXHIP_U16 && t->inten_dtype != NYXHIP_U32)
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "slide element type must be NYXHIP_U8 / U16 / U32");
    if (t->memory != NYXHIP_MEM_HOST && t->memory != NYXHIP_MEM_DEVICE) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad memory kind");
    if (t->n_tiles == 0) return NYXHIP_OK;
    if (t->width == 0 || t->height == 0 || t->width > kSlideMaxSide || t->height > kSlideMaxSide)
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "whole-slide mode takes slides of 1 to 65534 pixels a side (coordinates inside an ROI are 16-bit)");
    if (!t->inten) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null slide pointer");
    if (out_ld < (size_t)kImqCols) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream();
    const bool host = t->memory == NYXHIP_MEM_HOST;
    const uint32_t W = t->width, H = t->height;
    const uint64_t px = (uint64_t)W * H;
    const size_t in_bytes = (size_t)px * (size_t)t->inten_dtype;
    // ---- chunks of slides whose images and workspace fit the budget (the rule of nyxhip_featurize_slides)
    size_t budget = (size_t)t->max_device_bytes;
    if (budget == 0) {
        size_t fr = 0, tot = 0;
        HIP_TRY(ctx, hipMemGetInfo(&fr, &tot));
        const int sharers = std::max(1, g_ctx_on_device[ctx->device & 63].load());
        budget = (fr + ctx->d_tile.bytes + ctx->d_slot[0].bytes + ctx->d_slot[1].bytes) / 2 / (size_t)sharers;
    }
    const size_t per_slide = 8 * (size_t)kImqWords * (size_t)imq_slide_records(W, H) + 8 * (size_t)kImqCols + 64 + (host ? 2 * in_bytes : 0);
    if (per_slide > budget)
        return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "one slide and its workspace (" + std::to_string(per_slide >> 20) + " MiB) do not fit max_device_bytes");
    uint64_t chunk = budget / per_slide;
    if (host) chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(1, ((size_t)512 << 20) / in_bytes));      // <= 512 MiB per copy: the pipeline needs chunks
    if (chunk > t->n_tiles) chunk = t->n_tiles;
    if (host && t->n_tiles >= 4 && chunk > (t->n_tiles + 1) / 2) chunk = (t->n_tiles + 1) / 2;                // at least two chunks to overlap
    if (chunk > 65535) chunk = 65535;                      // the slide kernels spend a grid dimension on the slides of a chunk
    const uint64_t n_chunks = (t->n_tiles + chunk - 1) / chunk;

    if (!host) {
        for (uint64_t t0 = 0; t0 < t->n_tiles; t0 += chunk) {
            const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, t->n_tiles - t0);
            if (int rc = imq_slides_chunk(ctx, (const char*)t->inten + (size_t)t0 * in_bytes, t->inten_dtype, W, H, nt, s, out_table + t0 * out_ld, out_ld, st))
                return rc;
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return imq_check_status(ctx);
    }

    // ---- host slides: chunk c + 1 is copied through the pinned staging ring while chunk c is reduced
    if (int prc = ensure_copy_pipeline(ctx)) return prc;
    const size_t slot_need = (size_t)chunk * in_bytes + 512;
    for (int k = 0; k < (n_chunks > 1 ? 2 : 1); k++)
        HIP_TRY(ctx, ctx->d_slot[k].reserve(slot_need, st, imq_want(slot_need)));
    if (int grc = ensure_stage(ctx, (size_t)chunk * kImqCols * 8 + 256)) return grc;
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
        if (int rc = imq_slides_chunk(ctx, ctx->d_slot[k].p, t->inten_dtype, W, H, nt, s, d_out, (size_t)kImqCols, st)) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->slot_free[k], st));
        if (c + 1 < n_chunks)
            if (int urc = upload(c + 1)) return urc;                        // the next chunk's copy runs beside this chunk's kernels
        HIP_TRY(ctx, hipMemcpy2DAsync(out_table + t0 * out_ld, out_ld * sizeof(double), d_out, (size_t)kImqCols * sizeof(double), (size_t)kImqCols * sizeof(double), nt,
                                      hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));                             // the chunk's rows are on the host; d_stage is free for the next one
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
    return imq_check_status(ctx);
}

} // extern "C"
