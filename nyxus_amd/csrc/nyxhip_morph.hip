// nyxhip_morph.hip -- the 2-D morphology entries of include/nyxhip.h: column catalogue of a morphology mask, the launches over a
// device-resident batch (morph_device: the contour chain when PERIMETER is read, then morph_from_contours: roi_morph_kernel, its list
// launch over the boxes beyond the LDS carve), and nyxhip_morph_batch.  The tile entry (nyxhip_morph_tiles) lives with the tile path in nyxhip_tiles.hip.
#include "nyxhip_ctx.h"
#include "deferred_list.h"

using namespace nyxhip;

namespace nyxhip {

static const char* const kMorphBasicNames[kMorphBasicCols] = {
    "AREA_PIXELS_COUNT", "AREA_UM2", "CENTROID_X", "CENTROID_Y", "WEIGHTED_CENTROID_Y", "WEIGHTED_CENTROID_X", "MASS_DISPLACEMENT", "COMPACTNESS",
    "BBOX_YMIN", "BBOX_XMIN", "BBOX_HEIGHT", "BBOX_WIDTH", "DIAMETER_EQUAL_AREA", "EXTENT", "ASPECT_RATIO"};
static const char* const kMorphContourNames[kMorphContourCols] = {
    "PERIMETER", "DIAMETER_EQUAL_PERIMETER", "EDGE_MEAN_INTENSITY", "EDGE_STDDEV_INTENSITY", "EDGE_MAX_INTENSITY", "EDGE_MIN_INTENSITY",
    "EDGE_INTEGRATED_INTENSITY"};
static const char* const kMorphHullNames[kMorphHullCols] = {"CIRCULARITY", "CONVEX_HULL_AREA", "SOLIDITY"};

static bool morph_mask_ok(uint32_t m) { return m != 0 && (m & ~(uint32_t)NYXHIP_MORPH_ALL) == 0; }

int derive_batch_extrema(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t* max_px, uint32_t* max_area, uint32_t* max_side)
{
    hipStream_t st = ctx->stream();
    uint32_t ext[3] = {0, 0, 0};
    HIP_TRY(ctx, ctx->d_morph_ext.reserve(256, st));
    uint32_t* const d_ext = ctx->d_morph_ext.as<uint32_t>();
    HIP_TRY(ctx, hipMemsetAsync(d_ext, 0, 12, st));
    if (launch_nb_extrema(b->n_roi, b->px_offset, b->bbox_w, b->bbox_h, d_ext, st) != 0)
        return fail(ctx, NYXHIP_ERR_HIP, "morphology extrema kernel: launch failed");
    HIP_TRY(ctx, hipMemcpyAsync(ext, d_ext, 12, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *max_px = std::max(ext[0], 1u); *max_area = std::max(ext[1], 1u); *max_side = std::max(ext[2], 1u);
    return NYXHIP_OK;
}

int morph_device(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* d_ox, const uint32_t* d_oy, uint32_t morph, const nyxhip_settings* s,
                 double* d_out, size_t ld, uint32_t max_px, uint32_t max_area, uint32_t max_side)
{
    if (b->n_roi == 0) return NYXHIP_OK;
    if (max_px == 0 || max_area == 0 || max_side == 0)                        // a device batch without stated extrema: derive them
        if (int erc = derive_batch_extrema(ctx, b, &max_px, &max_area, &max_side)) return erc;
    // ---- the contour chain, unchanged and alone (no reader): PERIMETER and the EDGE_* columns read its workspace -------------------
    MomArgs m;
    memset(&m, 0, sizeof(m));
    if (morph & (NYXHIP_MORPH_HULL | NYXHIP_MORPH_CONTOUR))
        if (int crc = launch_contour_families(ctx, b, 0, s, nullptr, 0, max_px, max_area, max_side, false, &m)) return crc;
    return morph_from_contours(ctx, b, d_ox, d_oy, morph, m, d_out, ld, max_area, max_side);
}

int morph_from_contours(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* d_ox, const uint32_t* d_oy, uint32_t morph, const MomArgs& m, double* d_out,
                        size_t ld, uint32_t max_area, uint32_t max_side)
{
    hipStream_t st = ctx->stream();
    const uint64_t n = b->n_roi;
    if (n == 0) return NYXHIP_OK;
    const bool need_tab = (morph & NYXHIP_MORPH_HULL) != 0, need_plane = (morph & NYXHIP_MORPH_CONTOUR) != 0;
    MorphArgs a;
    memset(&a, 0, sizeof(a));
    a.n_roi = n;
    a.px_offset = b->px_offset; a.x = b->x; a.y = b->y; a.inten = b->inten; a.bbox_w = b->bbox_w; a.bbox_h = b->bbox_h;
    a.origin_x = d_ox; a.origin_y = d_oy;
    a.ws_contour = m.ws_contour; a.n_contour = m.n_contour;
    a.out = d_out; a.ld = ld; a.status = ctx->d_status.as<int>();
    a.morph = morph;
    a.col_basic = 0;
    a.col_contour = morph_n_columns(morph & NYXHIP_MORPH_BASIC);
    a.col_hull = morph_n_columns(morph & (NYXHIP_MORPH_BASIC | NYXHIP_MORPH_CONTOUR));
    a.col_extrema = morph_n_columns(morph & (NYXHIP_MORPH_BASIC | NYXHIP_MORPH_CONTOUR | NYXHIP_MORPH_HULL));
    // LDS from the batch extrema: a column table up to the widest box, a plane up to the largest box
    a.cols_cap = need_tab ? std::min<uint32_t>(kMorphColsLds, (std::min<uint32_t>(max_side, 65535u) + 7u) & ~7u) : 0u;
    a.plane_cap = need_plane ? std::min<uint32_t>(kMorphPlaneLds, (max_area + 3u < max_area ? max_area : max_area + 3u) & ~3u) : 0u;
    const bool may_defer = (need_tab && max_side > a.cols_cap) || (need_plane && max_area > a.plane_cap);
    a.defer_big = may_defer ? 1u : 0u;
    if (launch_roi_morph(a, st, (uint32_t)n) != 0)
        return fail(ctx, NYXHIP_ERR_HIP, "morphology kernel: launch failed");
    if (!may_defer) return NYXHIP_OK;
    DeferredList big;
    if (int rc = deferred_build(ctx, "morphology", ctx->d_morph.list, n,
                                MorphBig{b->bbox_w, b->bbox_h, need_tab ? a.cols_cap : 0xFFFFFFFFu, need_plane ? a.plane_cap : 0xFFFFFFFFu}, st, big))
        return rc;
    if (int rc = deferred_count(ctx, big, st)) return rc;
    if (!big.hdr[0]) return NYXHIP_OK;
    MorphArgs aw = a;
    aw.defer_big = 0;
    aw.ws_cols = need_tab ? (std::min<uint32_t>(big.hdr[1], 65535u) + 31u) & ~31u : 0u;
    aw.ws_cells = need_plane ? ((uint64_t)big.hdr[2] + 63) & ~63ull : 0ull;
    aw.ws_stride = (((uint64_t)kMorphBytesPerCol * aw.ws_cols + 255) & ~255ull) + ((4ull * aw.ws_cells + 255) & ~255ull);
    return deferred_chunks(ctx, "morphology", big, aw.ws_stride, (size_t)1 << 30, ctx->d_morph.ws, st, [&](const uint32_t* list, uint32_t count) {
        aw.ws = ctx->d_morph.ws.as<unsigned char>(); aw.roi_index = list;
        return launch_roi_morph(aw, st, count) != 0 ? fail(ctx, NYXHIP_ERR_HIP, "morphology kernel: launch failed") : NYXHIP_OK;
    });
}

} // namespace nyxhip

extern "C" {

int nyxhip_morph_n_columns(uint32_t morph_mask)
{
    return morph_mask_ok(morph_mask) ? morph_n_columns(morph_mask) : -1;
}

int nyxhip_morph_column_name(uint32_t morph_mask, int col, char* buf, size_t buf_len)
{
    if (!buf || buf_len == 0 || !morph_mask_ok(morph_mask) || col < 0 || col >= morph_n_columns(morph_mask)) return NYXHIP_ERR_INVALID_ARG;
    if (morph_mask & NYXHIP_MORPH_BASIC) {
        if (col < kMorphBasicCols) { snprintf(buf, buf_len, "%s", kMorphBasicNames[col]); return NYXHIP_OK; }
        col -= kMorphBasicCols;
    }
    if (morph_mask & NYXHIP_MORPH_CONTOUR) {
        if (col < kMorphContourCols) { snprintf(buf, buf_len, "%s", kMorphContourNames[col]); return NYXHIP_OK; }
        col -= kMorphContourCols;
    }
    if (morph_mask & NYXHIP_MORPH_HULL) {
        if (col < kMorphHullCols) { snprintf(buf, buf_len, "%s", kMorphHullNames[col]); return NYXHIP_OK; }
        col -= kMorphHullCols;
    }
    snprintf(buf, buf_len, "EXTREMA_P%d_%c", col / 2 + 1, (col & 1) ? 'Y' : 'X');
    return NYXHIP_OK;
}

int nyxhip_morph_batch(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y, uint32_t morph_mask,
                       const nyxhip_settings* s, double* out, size_t ld)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (!b || !s || !out) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null batch / settings / out_table");
    if (!morph_mask_ok(morph_mask)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad morphology mask");
    if ((origin_x == nullptr) != (origin_y == nullptr))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "origin_x and origin_y must both be given or both NULL");
    if (b->n_roi && (!b->px_offset || !b->x || !b->y || !b->inten || !b->bbox_w || !b->bbox_h))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "batch has null array pointers");
    const int n_cols = morph_n_columns(morph_mask);
    if (ld < (size_t)n_cols) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    if (b->n_roi > 0x7FFFFFFFull) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "too many ROIs in one batch");
    if (b->memory != NYXHIP_MEM_DEVICE && b->memory != NYXHIP_MEM_HOST) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad batch->memory");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->n_roi == 0) return NYXHIP_OK;
    hipStream_t st = ctx->stream();
    if (b->memory == NYXHIP_MEM_DEVICE) {
        const bool hinted = b->max_px != 0 && b->max_bbox_area != 0 && b->max_bbox_side != 0;
        if (int rc = morph_device(ctx, b, origin_x, origin_y, morph_mask, s, out, ld, hinted ? b->max_px : 0, hinted ? b->max_bbox_area : 0,
                                  hinted ? b->max_bbox_side : 0))
            return rc;
        return nyxhip_sync(ctx);
    }
    // host batch: derive extrema, check the CSR arrays, stage the arrays into one device slab, run, copy the table back
    const uint64_t nr = b->n_roi, npx = b->px_offset[nr];
    uint32_t max_px = 1, max_area = 1, max_side = 1;
    for (uint64_t r = 0; r < nr; r++) {
        if (b->px_offset[r + 1] < b->px_offset[r]) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "px_offset is not monotone");
        const uint64_t n = b->px_offset[r + 1] - b->px_offset[r], ar = (uint64_t)b->bbox_w[r] * b->bbox_h[r];
        if (n > 0xFFFFFFFFull || ar > 0xFFFFFFFFull) return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "ROI exceeds 2^32 pixels");
        max_px = std::max(max_px, (uint32_t)n);
        max_area = std::max(max_area, (uint32_t)ar);
        max_side = std::max(max_side, std::max(b->bbox_w[r], b->bbox_h[r]));
    }
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_off = 0, o_x = al(o_off + 8 * (nr + 1)), o_y = al(o_x + 2 * npx), o_i = al(o_y + 2 * npx), o_bw = al(o_i + 4 * npx),
                 o_bh = al(o_bw + 4 * nr), o_ox = al(o_bh + 4 * nr), o_oy = al(o_ox + (origin_x ? 4 * nr : 0)),
                 o_out = al(o_oy + (origin_x ? 4 * nr : 0)), total = al(o_out + 8ull * nr * (size_t)n_cols);
    if (int rc = ensure_stage(ctx, total)) return rc;
    char* const base = ctx->d_stage.as<char>();
    HIP_TRY(ctx, hipMemcpyAsync(base + o_off, b->px_offset, 8 * (nr + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_x, b->x, 2 * npx, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_y, b->y, 2 * npx, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_i, b->inten, 4 * npx, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_bw, b->bbox_w, 4 * nr, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_bh, b->bbox_h, 4 * nr, hipMemcpyHostToDevice, st));
    if (origin_x) {
        HIP_TRY(ctx, hipMemcpyAsync(base + o_ox, origin_x, 4 * nr, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(base + o_oy, origin_y, 4 * nr, hipMemcpyHostToDevice, st));
    }
    nyxhip_batch d;
    memset(&d, 0, sizeof(d));
    d.n_roi = nr; d.memory = NYXHIP_MEM_DEVICE;
    d.px_offset = (const uint64_t*)(base + o_off);
    d.x = (const uint16_t*)(base + o_x); d.y = (const uint16_t*)(base + o_y); d.inten = (const uint32_t*)(base + o_i);
    d.bbox_w = (const uint32_t*)(base + o_bw); d.bbox_h = (const uint32_t*)(base + o_bh);
    double* const d_out = (double*)(base + o_out);
    if (int rc = morph_device(ctx, &d, origin_x ? (const uint32_t*)(base + o_ox) : nullptr, origin_x ? (const uint32_t*)(base + o_oy) : nullptr,
                              morph_mask, s, d_out, (size_t)n_cols, max_px, max_area, max_side))
        return rc;
    HIP_TRY(ctx, hipMemcpy2DAsync(out, ld * sizeof(double), d_out, (size_t)n_cols * sizeof(double), (size_t)n_cols * sizeof(double), nr,
                                  hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return check_status(ctx);
}

} // extern "C"
