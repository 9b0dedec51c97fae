// nyxhip_morph.hip -- the 2-D morphology entries of include/nyxhip.h: column catalogue of a morphology mask, the launches over a
// device-resident batch (morph_device: the contour chain when PERIMETER is read, then morph_from_contours: roi_morph_kernel, its list
// launch over the boxes beyond the LDS carve), and nyxhip_morph_batch.  The tile entry (nyxhip_morph_tiles) lives with the tile path in nyxhip_tiles.hip.
#include "nyxhip_ctx.h"
#include "deferred_list.h"
#include "batch_stage.h"

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
    if (ctx && !morph_mask_ok(morph_mask)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad morphology mask");
    BatchSpec sp{kReadXY | kReadInten | kReadBox, "batch has null array pointers", morph_n_columns(morph_mask)};
    sp.origin_x = origin_x; sp.origin_y = origin_y;
    if (int rc = batch_check(ctx, sp, b, s, out, ld)) return rc;
    return batch_run(ctx, sp, b, out, ld, [&](const StagedBatch& g) {
        // the extrema: a host batch's at least 1 each (known), a device batch's complete statement, else 0 (morph_device derives them)
        auto known = [&](uint32_t v) { return g.hinted ? std::max(v, 1u) : 0u; };
        return morph_device(ctx, &g.d, g.d_ox, g.d_oy, morph_mask, s, g.d_out, g.ld, known(g.max_px), known(g.max_area), known(g.max_side));
    });
}

} // extern "C"
