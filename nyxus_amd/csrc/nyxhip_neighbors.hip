// nyxhip_neighbors.hip -- the neighbor entries of include/nyxhip.h: column names, the launches over a device-resident batch
// (neighbors_device: the contour chain, then neighbors_from_contours: geometry table, candidate lists, narrow phase, closing), the batch
// entry of the classes that relate the ROIs of an image (image_batch_entry) and nyxhip_neighbors_batch.  The tile entry
// (nyxhip_neighbors_tiles) lives with the tile path in nyxhip_tiles.hip.
#include "nyxhip_ctx.h"

using namespace nyxhip;

namespace nyxhip {

static const char* const kNeighborNames[kNeighborCols] = {
    "NUM_NEIGHBORS", "PERCENT_TOUCHING", "CLOSEST_NEIGHBOR1_DIST", "CLOSEST_NEIGHBOR1_ANG", "CLOSEST_NEIGHBOR2_DIST", "CLOSEST_NEIGHBOR2_ANG",
    "ANG_BW_NEIGHBORS_MEAN", "ANG_BW_NEIGHBORS_STDDEV", "ANG_BW_NEIGHBORS_MODE"};

namespace {

// the carve of nyxhip_ctx::d_nb_geo for n ROIs: geometry table, candidate counts and offsets, the three derived extrema
struct NbGeo {
    size_t o_box, o_cen, o_lo, o_hi, o_cnt, o_off, o_ext, need;
    explicit NbGeo(uint64_t n)
    {
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        o_box = 0; o_cen = al(o_box + 32 * n); o_lo = al(o_cen + 16 * n); o_hi = al(o_lo + 4 * n); o_cnt = al(o_hi + 4 * n);
        o_off = al(o_cnt + 4 * n); o_ext = al(o_off + 8 * (n + 1)); need = al(o_ext + 16);
    }
};

} // namespace

int neighbors_device(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* d_ox, const uint32_t* d_oy, const uint64_t* d_image_offset, uint64_t n_images,
                     const uint32_t* d_image_id, int32_t pixel_distance, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px,
                     uint32_t max_area, uint32_t max_side)
{
    hipStream_t st = ctx->stream();
    const uint64_t n = b->n_roi;
    if (n == 0) return NYXHIP_OK;
    const NbGeo G(n);
    HIP_TRY(ctx, ctx->d_nb_geo.reserve(G.need, st, G.need + G.need / 8));
    char* const g = ctx->d_nb_geo.as<char>();
    const size_t o_ext = G.o_ext;
    if (max_px == 0 || max_area == 0 || max_side == 0) {                      // a device batch without stated extrema: derive them
        uint32_t ext[3] = {0, 0, 0};
        HIP_TRY(ctx, hipMemsetAsync(g + o_ext, 0, 12, st));
        if (launch_nb_extrema(n, b->px_offset, b->bbox_w, b->bbox_h, (uint32_t*)(g + o_ext), st) != 0)
            return fail(ctx, NYXHIP_ERR_HIP, "neighbor extrema kernel: launch failed");
        HIP_TRY(ctx, hipMemcpyAsync(ext, g + o_ext, 12, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        max_px = ext[0]; max_area = ext[1]; max_side = ext[2];
    }
    // ---- the contour chain, unchanged: roi_contour_kernel with its big-box list chain, no reader ----------------------------------
    MomArgs m;
    if (int crc = launch_contour_families(ctx, b, 0, s, nullptr, 0, max_px, max_area, max_side, false, &m)) return crc;
    return neighbors_from_contours(ctx, b, d_ox, d_oy, d_image_offset, n_images, d_image_id, pixel_distance, m, d_out, ld);
}

int neighbors_from_contours(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* d_ox, const uint32_t* d_oy, const uint64_t* d_image_offset,
                            uint64_t n_images, const uint32_t* d_image_id, int32_t pixel_distance, const MomArgs& m, double* d_out, size_t ld)
{
    hipStream_t st = ctx->stream();
    const uint64_t n = b->n_roi;
    if (n == 0) return NYXHIP_OK;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    // ---- geometry table, candidate counts and offsets (sized by the ROI count) ------------------------------------------------
    const NbGeo G(n);
    HIP_TRY(ctx, ctx->d_nb_geo.reserve(G.need, st, G.need + G.need / 8));
    char* const g = ctx->d_nb_geo.as<char>();
    const size_t o_box = G.o_box, o_cen = G.o_cen, o_lo = G.o_lo, o_hi = G.o_hi, o_cnt = G.o_cnt, o_off = G.o_off;
    NbArgs a;
    memset(&a, 0, sizeof(a));
    a.n_roi = n;
    a.px_offset = b->px_offset; a.x = b->x; a.y = b->y; a.bbox_w = b->bbox_w; a.bbox_h = b->bbox_h; a.label = b->roi_label;
    a.origin_x = d_ox; a.origin_y = d_oy;
    a.image_offset = d_image_offset; a.n_images = n_images; a.image_id = d_image_id;
    a.ws_contour = m.ws_contour; a.n_contour = m.n_contour;
    a.radius = pixel_distance;
    a.box = (long long*)(g + o_box); a.cen = (double*)(g + o_cen); a.img_lo = (uint32_t*)(g + o_lo); a.img_hi = (uint32_t*)(g + o_hi);
    a.cand_count = (uint32_t*)(g + o_cnt); a.cand_off = (uint64_t*)(g + o_off);
    a.out = d_out; a.ld = ld; a.status = ctx->d_status.as<int>();
    int rc = launch_nb_geometry(a, st);
    if (rc == 0) rc = launch_nb_candidates_count(a, st);
    if (rc != 0) return fail(ctx, NYXHIP_ERR_HIP, std::string("neighbor geometry / candidate kernels: launch failed: ") + hipGetErrorString((hipError_t)rc));
    // ---- candidate lists (sized by their total: the one read-back of the call besides the contour chain's) ----------------------
    uint64_t total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, a.cand_off + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const size_t o_c = 0, o_min = al(o_c + 4 * total + 4), o_ang = al(o_min + 8 * total + 8), o_flag = al(o_ang + 2 * total + 2),
                 cand_need = al(o_flag + total + 1);
    HIP_TRY(ctx, ctx->d_nb_cand.reserve(cand_need, st, cand_need + cand_need / 8));
    char* const c = ctx->d_nb_cand.as<char>();
    a.cand = (uint32_t*)(c + o_c); a.cand_min = (unsigned long long*)(c + o_min); a.cand_ang = (uint16_t*)(c + o_ang); a.cand_flag = (uint8_t*)(c + o_flag);
    if (total) rc = launch_nb_candidates_fill(a, st);
    if (rc == 0) rc = launch_nb_narrow(a, st);
    if (rc == 0) rc = launch_nb_close(a, st);
    if (rc != 0) return fail(ctx, NYXHIP_ERR_HIP, std::string("neighbor kernels: launch failed: ") + hipGetErrorString((hipError_t)rc));
    return NYXHIP_OK;
}

// The batch entry of a class that relates the ROIs of an image to each other -- nyxhip_neighbors_batch, and nyxhip_hexpoly_batch which
// reads the neighbor count: argument checks, the device batch as it is, a host batch staged into one slab and its table copied back.
// n_cols columns come from device_fn.
int image_batch_entry(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y, const uint64_t* image_offset,
                      uint64_t n_images, int32_t pixel_distance, const nyxhip_settings* s, double* out, size_t ld, int n_cols, ImageBatchFn device_fn)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (!b || !s || !out) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null batch / settings / out_table");
    if (pixel_distance <= 0) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "pixel_distance must be greater than zero");
    if (pixel_distance > kNbMaxDistance)
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "pixel_distance beyond 46340: its square overflows the reference's int (neighbors.cpp:242)");
    if ((origin_x == nullptr) != (origin_y == nullptr))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "origin_x and origin_y must both be given or both NULL");
    if (b->n_roi && (!b->roi_label || !b->px_offset || !b->x || !b->y || !b->inten || !b->bbox_w || !b->bbox_h))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "batch has null array pointers (the neighbor entries read roi_label)");
    if (ld < (size_t)n_cols) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    if (b->n_roi > 0x7FFFFFFFull) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "too many ROIs in one batch");
    if (image_offset && n_images == 0) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "image_offset given with n_images == 0");
    if (b->memory != NYXHIP_MEM_DEVICE && b->memory != NYXHIP_MEM_HOST) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad batch->memory");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->n_roi == 0) return NYXHIP_OK;
    hipStream_t st = ctx->stream();
    if (b->memory == NYXHIP_MEM_DEVICE) {
        const bool hinted = b->max_px != 0 && b->max_bbox_area != 0 && b->max_bbox_side != 0;
        if (int rc = device_fn(ctx, b, origin_x, origin_y, image_offset, n_images, nullptr, pixel_distance, s, out, ld, hinted ? b->max_px : 0,
                               hinted ? b->max_bbox_area : 0, hinted ? b->max_bbox_side : 0))
            return rc;
        return nyxhip_sync(ctx);
    }
    // host batch: derive extrema, check the CSR arrays, stage the arrays into one device slab, run, copy the table back
    const uint64_t nr = b->n_roi, npx = b->px_offset[nr];
    uint32_t max_px = 0, max_area = 0, max_side = 0;
    for (uint64_t r = 0; r < nr; r++) {
        if (b->px_offset[r + 1] < b->px_offset[r]) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "px_offset is not monotone");
        const uint64_t n = b->px_offset[r + 1] - b->px_offset[r], ar = (uint64_t)b->bbox_w[r] * b->bbox_h[r];
        if (n > 0xFFFFFFFFull || ar > 0xFFFFFFFFull) return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "ROI exceeds 2^32 pixels");
        max_px = std::max(max_px, (uint32_t)n);
        max_area = std::max(max_area, (uint32_t)ar);
        max_side = std::max(max_side, std::max(b->bbox_w[r], b->bbox_h[r]));
    }
    if (image_offset) {
        if (image_offset[0] != 0 || image_offset[n_images] != nr) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "image_offset must run from 0 to n_roi");
        for (uint64_t k = 0; k < n_images; k++)
            if (image_offset[k + 1] < image_offset[k]) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "image_offset is not monotone");
    }
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_off = 0, o_x = al(o_off + 8 * (nr + 1)), o_y = al(o_x + 2 * npx), o_i = al(o_y + 2 * npx), o_bw = al(o_i + 4 * npx),
                 o_bh = al(o_bw + 4 * nr), o_lab = al(o_bh + 4 * nr), o_ox = al(o_lab + 4 * nr), o_oy = al(o_ox + (origin_x ? 4 * nr : 0)),
                 o_img = al(o_oy + (origin_x ? 4 * nr : 0)), o_out = al(o_img + (image_offset ? 8 * (n_images + 1) : 0)),
                 total = al(o_out + 8ull * nr * (size_t)n_cols);
    if (int rc = ensure_stage(ctx, total)) return rc;
    char* const base = ctx->d_stage.as<char>();
    HIP_TRY(ctx, hipMemcpyAsync(base + o_off, b->px_offset, 8 * (nr + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_x, b->x, 2 * npx, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_y, b->y, 2 * npx, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_i, b->inten, 4 * npx, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_bw, b->bbox_w, 4 * nr, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_bh, b->bbox_h, 4 * nr, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_lab, b->roi_label, 4 * nr, hipMemcpyHostToDevice, st));
    if (origin_x) {
        HIP_TRY(ctx, hipMemcpyAsync(base + o_ox, origin_x, 4 * nr, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(base + o_oy, origin_y, 4 * nr, hipMemcpyHostToDevice, st));
    }
    if (image_offset) HIP_TRY(ctx, hipMemcpyAsync(base + o_img, image_offset, 8 * (n_images + 1), hipMemcpyHostToDevice, st));
    nyxhip_batch d;
    memset(&d, 0, sizeof(d));
    d.n_roi = nr; d.memory = NYXHIP_MEM_DEVICE;
    d.roi_label = (const uint32_t*)(base + o_lab); d.px_offset = (const uint64_t*)(base + o_off);
    d.x = (const uint16_t*)(base + o_x); d.y = (const uint16_t*)(base + o_y); d.inten = (const uint32_t*)(base + o_i);
    d.bbox_w = (const uint32_t*)(base + o_bw); d.bbox_h = (const uint32_t*)(base + o_bh);
    double* const d_out = (double*)(base + o_out);
    if (int rc = device_fn(ctx, &d, origin_x ? (const uint32_t*)(base + o_ox) : nullptr, origin_x ? (const uint32_t*)(base + o_oy) : nullptr,
                           image_offset ? (const uint64_t*)(base + o_img) : nullptr, n_images, nullptr, pixel_distance, s, d_out,
                           (size_t)n_cols, max_px, max_area, max_side))
        return rc;
    HIP_TRY(ctx, hipMemcpy2DAsync(out, ld * sizeof(double), d_out, (size_t)n_cols * sizeof(double), (size_t)n_cols * sizeof(double), nr,
                                  hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return check_status(ctx);
}

} // namespace nyxhip

extern "C" {

int nyxhip_neighbor_column_name(int col, char* buf, size_t buf_len)
{
    if (!buf || buf_len == 0 || col < 0 || col >= kNeighborCols) return NYXHIP_ERR_INVALID_ARG;
    snprintf(buf, buf_len, "%s", kNeighborNames[col]);
    return NYXHIP_OK;
}

int nyxhip_neighbors_batch(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y, const uint64_t* image_offset,
                           uint64_t n_images, int32_t pixel_distance, const nyxhip_settings* s, double* out, size_t ld)
{
    return image_batch_entry(ctx, b, origin_x, origin_y, image_offset, n_images, pixel_distance, s, out, ld, kNeighborCols, neighbors_device);
}

} // extern "C"
