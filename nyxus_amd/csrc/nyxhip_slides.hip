// nyxhip_slides.hip -- whole-slide mode: nyxhip_featurize_slides, one ROI per slide and no label image.
//
// The reference reaches this mode through featurize_files(..., single_roi = True) and a featurize_directory() without a label
// directory (the reference's src/nyx/workflow_2d_whole.cpp:36-213, reduce_trivial_rois.cpp:798-819, slideprops.cpp:101-254): the
// ROI is the image.  Row t of the table has the bits of nyxhip_featurize_batch on the one-ROI batch whose cloud is slide t in
// row-major order, whose box is the image and whose extrema -- the ROI's and the slide's -- are taken over all pixels.
//
// Per chunk of slides resident on the device: slide extrema and per-ROI rows (roi_slide.hip), then one of two chains per slide.
//   dense chain  INTENSITY / GLCM on a slide of the largest size class with a range below kLargeRangeMax: the several-workgroups-per-ROI
//                kernels of roi_large.hip read the image itself (large_load_dense_kernel) -- no cloud, no coordinates
//   cloud route  everything else: the row-major cloud (slide_cloud_kernel), then the device batch dispatch every other entry ends in
//                (launch_device), so every family keeps its own size-class kernels and limits
// Both end in the same integer tables and the same finishing kernels, so the rows do not depend on the choice.
#include "nyxhip_ctx.h"

using namespace nyxhip;

namespace {

constexpr uint32_t kSlideFams = 0x3FFu;            // bits 0-9: NYXHIP_FAM_ALL without the two moment classes
constexpr uint32_t kSlideMaxSide = 65534;          // the batch ABI's coordinates are 16-bit
constexpr uint32_t kValidFams = NYXHIP_FAM_ALL | NYXHIP_FAM_RADIAL | kOutline | kCaliper | NYXHIP_FAM_CHORDS | kEllipseErosion | kCircleGeodetic;

size_t slide_want(size_t need) { return need + need / 8 + (1 << 16); }

// Device bytes of one slide besides its staging copies: the cloud, the rows, the table row.
size_t slide_ws_bytes(uint64_t px, int n_cols) { return 8 * (size_t)px + 8 * (size_t)n_cols + 64; }

// nt slides resident on the device -> nt rows at d_out (device, leading dimension ld), enqueued on st.
int slides_chunk(nyxhip_ctx* ctx, const void* d_inten, int dt, uint32_t W, uint32_t H, uint32_t nt, uint32_t mask, const nyxhip_settings* s,
                 double* d_out, size_t ld, hipStream_t st)
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint64_t px = (uint64_t)W * H, npx = px * nt;
    size_t o = 0;
    const size_t o_off = o; o = al(o + 8 * ((size_t)nt + 1));
    const size_t o_smin = o; o = al(o + 8 * (size_t)nt);
    const size_t o_smax = o; o = al(o + 8 * (size_t)nt);
    size_t o_u[5]; for (int i = 0; i < 5; i++) { o_u[i] = o; o = al(o + 4 * (size_t)nt); }
    HIP_TRY(ctx, ctx->d_tile.reserve(o, st, slide_want(o)));
    char* const base = ctx->d_tile.as<char>();
    SlideRows R{(uint32_t*)(base + o_u[0]), (uint64_t*)(base + o_off), (uint32_t*)(base + o_u[1]), (uint32_t*)(base + o_u[2]),
                (uint32_t*)(base + o_u[3]), (uint32_t*)(base + o_u[4]), (double*)(base + o_smin), (double*)(base + o_smax)};
    if (int rc = launch_slide_headers(d_inten, dt, W, H, nt, R, st))
        return fail(ctx, NYXHIP_ERR_HIP, std::string("slide extrema launch failed: ") + hipGetErrorString((hipError_t)rc));
    // the extrema on the host: the batch extrema of the dispatch, as a host batch states them
    std::vector<uint32_t> hmm(2 * (size_t)nt);
    HIP_TRY(ctx, hipMemcpyAsync(hmm.data(), R.vmin, 4 * (size_t)nt, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(hmm.data() + nt, R.vmax, 4 * (size_t)nt, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    // ---- which chain takes a slide is a function of the slide and the mask alone.  The dense chain (launch_dense_slides: the
    // several-workgroups-per-ROI kernels of roi_large.hip reading the image itself) takes INTENSITY / GLCM requests on slides of the
    // largest size class whose intensity range the histogram workspace holds -- exactly the ROIs those kernels serve behind the batch
    // entry; everything else gets its row-major cloud and goes through the device batch dispatch.  Runs of consecutive slides that
    // share the answer share a launch group; both kinds index the chunk by the absolute CSR offsets of the rows.
    const bool dense_mask = (mask & ~(uint32_t)(NYXHIP_FAM_INTENSITY | NYXHIP_FAM_GLCM)) == 0;
    const bool class4 = roi_class((uint32_t)px, W, H, 0) / 2 == kSizeClasses - 1;
    auto dense_ok = [&](uint32_t t) { return dense_mask && class4 && hmm[nt + t] - hmm[t] < kLargeRangeMax; };
    const uint16_t *cx = nullptr, *cy = nullptr; const uint32_t* cv = nullptr;
    bool clouds_made = false;
    for (uint32_t t0 = 0; t0 < nt;) {
        const bool dense = dense_ok(t0);
        uint32_t t1 = t0 + 1;
        while (t1 < nt && dense_ok(t1) == dense) t1++;
        const uint32_t n = t1 - t0;
        uint32_t max_range = 0, vmax = 0;
        uint64_t range1 = 0;
        for (uint32_t t = t0; t < t1; t++) {
            max_range = std::max(max_range, hmm[nt + t] - hmm[t]); vmax = std::max(vmax, hmm[nt + t]);
            range1 += (uint64_t)(hmm[nt + t] - hmm[t]) + 1;
        }
        nyxhip_batch b;
        memset(&b, 0, sizeof(b));
        b.n_roi = n; b.roi_label = R.label + t0; b.px_offset = R.px_offset + t0;
        b.bbox_w = R.bbox_w + t0; b.bbox_h = R.bbox_h + t0; b.min_inten = R.vmin + t0; b.max_inten = R.vmax + t0;
        b.slide_min = R.slide_min + t0; b.slide_max = R.slide_max + t0;
        b.memory = NYXHIP_MEM_DEVICE;
        double* const out = d_out + (size_t)t0 * ld;
        bool served = false;
        if (dense) {
            const Extrema E{(uint32_t)px, (uint32_t)px, max_range, std::max(W, H), vmax, false};
            const ClassTotals tot{px * n, px * n, range1};
            if (int rc = launch_dense_slides(ctx, &b, d_inten, dt, mask, s, out, ld, E, tot, &served)) return rc;
        }
        if (!served) {
            if (!clouds_made) {
                size_t c = 0;
                const size_t o_cx = c; c = al(c + 2 * npx);
                const size_t o_cy = c; c = al(c + 2 * npx);
                const size_t o_cv = c; c = al(c + 4 * npx);
                HIP_TRY(ctx, ctx->d_cloud.reserve(c, st, slide_want(c)));
                char* const cb = ctx->d_cloud.as<char>();
                cx = (const uint16_t*)(cb + o_cx); cy = (const uint16_t*)(cb + o_cy); cv = (const uint32_t*)(cb + o_cv);
                clouds_made = true;
            }
            // (the clouds of the run, at their place in the chunk's cloud: slide t owns [t * px, (t + 1) * px))
            if (int rc = launch_slide_clouds(d_inten, dt, W, H, t0, n, (uint16_t*)cx, (uint16_t*)cy, (uint32_t*)cv, st))
                return fail(ctx, NYXHIP_ERR_HIP, std::string("slide cloud launch failed: ") + hipGetErrorString((hipError_t)rc));
            b.x = cx; b.y = cy; b.inten = cv;
            const bool small = px <= kClassPx[0] && W <= kClassSide[0] && H <= kClassSide[0];
            ctx->census_small = small ? n : 0; ctx->census_total = n; ctx->census_pending = 0;   // (as the host batch entry counts its ROIs)
            if (int rc = launch_device(ctx, &b, mask, s, out, ld, (uint32_t)px, (uint32_t)px, max_range, std::max(W, H))) return rc;
        }
        t0 = t1;
    }
    return NYXHIP_OK;
}

} // namespace

extern "C" {

int nyxhip_featurize_slides(nyxhip_ctx* ctx, const nyxhip_tiles* t, uint32_t family_mask, const nyxhip_settings* s, double* out_table, size_t out_ld)
{
    if (!t || !s || !out_table) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null slides / settings / out_table");
    if (t->label) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "whole-slide mode takes no label image: slides->label must be NULL");
    if (family_mask == 0 || (family_mask & ~kValidFams)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad family mask");
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (family_mask & ~kSlideFams)
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "whole-slide mode serves the intensity, GLCM, GLRLM, GLSZM, NGTDM, GABOR, ZERNIKE2D, GLDZM, GLDM and NGLDM "
                                                 "families (bits 0-9): the moment classes weight differently in this mode, and the contour-based families are not part of it");
    if (t->inten_dtype != NYXHIP_U8 && t->inten_dtype != NYXHIP_U16 && t->inten_dtype != NYXHIP_U32)
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "slide element type must be NYXHIP_U8 / U16 / U32");
    if (t->memory != NYXHIP_MEM_HOST && t->memory != NYXHIP_MEM_DEVICE) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad memory kind");
    if (t->n_tiles == 0) return NYXHIP_OK;
    if (t->width == 0 || t->height == 0 || t->width > kSlideMaxSide || t->height > kSlideMaxSide)
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "whole-slide mode takes slides of 1 to 65534 pixels a side (coordinates inside an ROI are 16-bit)");
    if (!t->inten) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null slide pointer");
    std::string why;
    if (!settings_ok(s, family_mask, why)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, why);
    const int n_cols = nyxhip_n_columns(family_mask, s);
    if ((int)out_ld < n_cols) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream();
    const bool host = t->memory == NYXHIP_MEM_HOST;
    const uint32_t W = t->width, H = t->height;
    const uint64_t px = (uint64_t)W * H;
    const size_t in_bytes = (size_t)px * (size_t)t->inten_dtype;
    // ---- chunks of slides whose images and workspace fit the budget (the tile path's rule, nyxhip_tiles::max_device_bytes)
    size_t budget = (size_t)t->max_device_bytes;
    if (budget == 0) {
        size_t fr = 0, tot = 0;
        HIP_TRY(ctx, hipMemGetInfo(&fr, &tot));
        const int sharers = std::max(1, g_ctx_on_device[ctx->device & 63].load());
        budget = (fr + ctx->d_tile.bytes + ctx->d_cloud.bytes + ctx->d_slot[0].bytes + ctx->d_slot[1].bytes) / 2 / (size_t)sharers;
    }
    const size_t per_slide = slide_ws_bytes(px, n_cols) + (host ? 2 * in_bytes : 0);
    if (per_slide > budget)
        return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "one slide and its workspace (" + std::to_string(per_slide >> 20) + " MiB) do not fit max_device_bytes");
    uint64_t chunk = budget / per_slide;
    if (host) chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(1, ((size_t)512 << 20) / in_bytes));      // <= 512 MiB per copy: the pipeline needs chunks
    if (chunk > t->n_tiles) chunk = t->n_tiles;
    if (host && t->n_tiles >= 4 && chunk > (t->n_tiles + 1) / 2) chunk = (t->n_tiles + 1) / 2;                // at least two chunks to overlap
    if (chunk > 65535) chunk = 65535;                      // the slide kernels spend grid.y on the slides of a chunk
    const uint64_t n_chunks = (t->n_tiles + chunk - 1) / chunk;

    if (!host) {
        for (uint64_t t0 = 0; t0 < t->n_tiles; t0 += chunk) {
            const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, t->n_tiles - t0);
            if (int rc = slides_chunk(ctx, (const char*)t->inten + (size_t)t0 * in_bytes, t->inten_dtype, W, H, nt, family_mask, s, out_table + t0 * out_ld, out_ld, st))
                return rc;
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return check_status(ctx);
    }

    // ---- host slides: chunk c + 1 is copied through the pinned staging ring while chunk c is reduced -------------------------------
    if (int prc = ensure_copy_pipeline(ctx)) return prc;
    const size_t slot_need = (size_t)chunk * in_bytes + 512;
    for (int k = 0; k < (n_chunks > 1 ? 2 : 1); k++)
        HIP_TRY(ctx, ctx->d_slot[k].reserve(slot_need, st, slide_want(slot_need)));
    if (int grc = ensure_stage(ctx, (size_t)chunk * n_cols * 8 + 256)) return grc;
    auto upload = [&](uint64_t c) -> int {                                  // chunk c -> slot c & 1 on the copy stream
        const int k = (int)(c & 1);
        const uint64_t t0 = c * chunk;
        const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, t->n_tiles - t0);
        if (c >= 2) HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->slot_free[k], 0));      // the kernels of chunk c - 2 have let go of the slot
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
        if (int rc = slides_chunk(ctx, ctx->d_slot[k].p, t->inten_dtype, W, H, nt, family_mask, s, d_out, (size_t)n_cols, st)) return rc;
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
