// nyxhip_neighbors.hip -- the neighbor entries of include/nyxhip.h: column names, the launches over a device-resident batch
// (neighbors_device: the contour chain, then neighbors_from_contours: geometry table, candidate lists, narrow phase, closing), the batch
// entry of the classes that relate the ROIs of an image (image_batch_entry) and nyxhip_neighbors_batch.  The tile entry
// (nyxhip_neighbors_tiles) lives with the tile path in nyxhip_tiles.hip.
#include "nyxhip_ctx.h"
#include "batch_stage.h"

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
// reads the neighbor count: the checks and the staging of batch_stage.h around device_fn, which gives n_cols columns.
int image_batch_entry(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y, const uint64_t* image_offset,
                      uint64_t n_images, int32_t pixel_distance, const nyxhip_settings* s, double* out, size_t ld, int n_cols, ImageBatchFn device_fn)
{
    BatchSpec sp{kReadLabel | kReadXY | kReadInten | kReadBox, "batch has null array pointers (the neighbor entries read roi_label)", n_cols};
    sp.origin_x = origin_x; sp.origin_y = origin_y; sp.image_offset = image_offset; sp.n_images = n_images;
    if (int rc = batch_check(ctx, sp, b, s, out, ld)) return rc;
    if (int rc = pixel_distance_check(ctx, pixel_distance)) return rc;
    return batch_run(ctx, sp, b, out, ld, [&](const StagedBatch& g) {
        // the extrema: a host batch's as walked, a device batch's complete statement; any 0: device_fn derives them
        return device_fn(ctx, &g.d, g.d_ox, g.d_oy, g.d_image_offset, n_images, nullptr, pixel_distance, s, g.d_out, g.ld, g.hinted ? g.max_px : 0,
                         g.hinted ? g.max_area : 0, g.hinted ? g.max_side : 0);
    });
}

int pixel_distance_check(nyxhip_ctx* ctx, int32_t pixel_distance)
{
    if (pixel_distance <= 0) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "pixel_distance must be greater than zero");
    if (pixel_distance > kNbMaxDistance)
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "pixel_distance beyond 46340: its square overflows the reference's int (neighbors.cpp:242)");
    return NYXHIP_OK;
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
