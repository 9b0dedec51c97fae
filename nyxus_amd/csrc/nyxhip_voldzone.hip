// nyxhip_voldzone.hip -- the volume distance-zone entries of include/nyxhip.h: the column catalogue of the distance-zone mask
// (nyxhip_voldzone_n_columns, nyxhip_voldzone_column_name) and nyxhip_featurize_volumes_dzones: checks, then (vol_host.h) the staging of
// a host batch; here the largest box sides of the batch (they size the tables and the grids), the chunks of ROIs under the device budget,
// the binned boxes (launch_vol_bin of roi_vol.hip) and the launches of roi_voldzone.hip.
#include "nyxhip_ctx.h"
#include "vol_host.h"
#include "roi_vol.h"
#include "roi_voldzone.h"

using namespace nyxhip;

namespace {

// save_value order (3d_gldzm.cpp:550-570) under the reference's user-facing names (featureset.cpp:842-859)
const char* const kGldzmNames[kVdzCols] = {"SDE", "LDE", "LGLZE", "HGLZE", "SDLGLE", "SDHGLE", "LDLGLE", "LDHGLE", "GLNU", "GLNUN", "ZDNU", "ZDNUN", "ZP", "GLM", "GLV", "ZDM",
                                           "ZDV", "ZDE"};

bool dzone_mask_ok(uint32_t m) { return m == (uint32_t)NYXHIP_VDZ_GLDZM; }
size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
const std::string kCapText = "volume distance zones: a level is a table row and a byte of the binned box, up to NYXHIP_VOLDZONE_MAX_LEVELS = " + std::to_string(kVzLevelCap) + " levels";

int voldzone_check_status(nyxhip_ctx* ctx)
{
    const int rc = check_status(ctx);
    if (rc == NYXHIP_ERR_UNSUPPORTED)
        return fail(ctx, rc, kCapText + ", and an ROI has a larger intensity (IBSI mode, or coarse_gray_depth = 0: the levels are the intensities)");
    if (rc == NYXHIP_ERR_ROI_TOO_LARGE)
        return fail(ctx, rc, "volume distance zones: an ROI exceeds the stated extrema, a box side of " + std::to_string(kVolMaxSide) + " or " + std::to_string(kVolMaxCells) + " cells");
    if (rc == NYXHIP_ERR_INVALID_ARG) return fail(ctx, rc, "volume distance zones: a voxel lies outside its box");
    if (rc == NYXHIP_ERR_INTERNAL) return fail(ctx, rc, "volume distance zones: a device loop reached the bound derived from its box (a label chase or a zone metric)");
    return rc;
}

// the ROIs of a device-resident batch -> d_out [n_roi x ld] (device), in chunks whose workspace fits the budget; enqueued on the stream
int voldzone_device(nyxhip_ctx* ctx, const nyxhip_batch3d& b, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px, uint32_t max_cells)
{
    hipStream_t st = ctx->stream();
    VoldzoneArgs a;
    memset(&a, 0, sizeof(a));
    a.px_offset = b.px_offset;
    a.bbox_w = b.bbox_w; a.bbox_h = b.bbox_h; a.bbox_d = b.bbox_d; a.vmin = b.min_inten; a.vmax = b.max_inten;
    a.g = s->ibsi ? 0 : s->grey_depth;                     // 3d_gldzm.cpp:68-73: n_levels is never set
    a.rows = (a.g ? (uint32_t)abs(a.g) : kVzLevelCap) + 1u;
    a.soft_nan = s->soft_nan; a.out = d_out; a.ld = ld;
    a.status = ctx->d_status.as<int>();
    a.max_cells = max_cells ? max_cells : 1u;
    a.box_stride = al256(a.max_cells);
    // the tables are sized by the largest min(w, h) of the batch, the grids by its largest sides: one copy of the boxes, whatever
    // extrema are stated
    {
        const uint64_t nr = b.n_roi;
        std::vector<uint32_t> whd(3 * nr);
        HIP_TRY(ctx, hipMemcpyAsync(whd.data(), b.bbox_w, 4 * nr, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(whd.data() + nr, b.bbox_h, 4 * nr, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(whd.data() + 2 * nr, b.bbox_d, 4 * nr, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        a.side_max[0] = a.side_max[1] = a.side_max[2] = 1u;
        a.pitch_max = vdz_pitch(1u, 1u);
        for (uint64_t r = 0; r < nr; r++) {
            const uint32_t w = whd[r], h = whd[nr + r], d = whd[2 * nr + r];
            if (w > kVolMaxSide || h > kVolMaxSide || d > kVolMaxSide || (uint64_t)w * h * d > (uint64_t)a.max_cells) continue;   // (refused on the device)
            a.side_max[0] = std::max(a.side_max[0], w);
            a.side_max[1] = std::max(a.side_max[1], h);
            a.side_max[2] = std::max(a.side_max[2], d);
            a.pitch_max = std::max(a.pitch_max, vdz_pitch(w, h));
        }
    }
    a.tab_stride = al256(4 * ((size_t)kVdzHead + (size_t)a.rows * a.pitch_max)) >> 2;
    a.cell_stride = al256(4 * (size_t)a.max_cells) >> 2;
    a.dist_stride = al256(2 * (size_t)a.max_cells) >> 1;
    const size_t per_roi = a.box_stride + 4 * a.tab_stride + 2 * a.dist_stride + 8 * a.cell_stride;
    size_t budget = 0;
    if (int rc = vol_budget(ctx, &b, ctx->d_vol.bytes, budget)) return rc;
    if (per_roi > budget)
        return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "volume distance zones: the workspace of one ROI (" + std::to_string(per_roi) + " bytes) does not fit max_device_bytes");
    const uint64_t chunk = std::min<uint64_t>(budget / per_roi, std::min<uint64_t>(65535, b.n_roi));   // (a grid dimension counts the ROIs of a chunk)
    HIP_TRY(ctx, ctx->d_vol.reserve((size_t)chunk * per_roi, st));
    // the workspace: the tables of the chunk (one memset), then labels, minima, distances, boxes
    char* const base = ctx->d_vol.as<char>();
    a.tab = (uint32_t*)base;
    a.label = a.tab + chunk * a.tab_stride;
    a.zmin = a.label + chunk * a.cell_stride;
    a.dist = (uint16_t*)(a.zmin + chunk * a.cell_stride);
    unsigned char* const boxes = (unsigned char*)(a.dist + chunk * a.dist_stride);
    a.box = boxes;
    for (uint64_t r0 = 0; r0 < b.n_roi; r0 += chunk) {
        a.roi0 = r0; a.n_roi = std::min<uint64_t>(chunk, b.n_roi - r0);
        HIP_TRY(ctx, hipMemsetAsync(base, 0, 4 * (size_t)chunk * a.tab_stride, st));
        VolArgs v;                                         // vol_bin_kernel: bin_intensities_3d with the class's greyInfo
        memset(&v, 0, sizeof(v));
        v.roi0 = a.roi0; v.n_roi = a.n_roi; v.px_offset = b.px_offset; v.x = b.x; v.y = b.y; v.z = b.z; v.inten = b.inten;
        v.bbox_w = a.bbox_w; v.bbox_h = a.bbox_h; v.bbox_d = a.bbox_d; v.vmin = a.vmin; v.vmax = a.vmax;
        v.grey_info = a.g; v.status = a.status; v.boxes = boxes; v.box_stride = a.box_stride;
        v.max_cells = a.max_cells; v.max_px = max_px ? max_px : 1u;
        HIP_TRY(ctx, hipMemsetAsync(boxes, vol_background_level(a.g), (size_t)a.n_roi * a.box_stride, st));
        if (int rc = launch_vol_bin(v, st)) return fail(ctx, NYXHIP_ERR_HIP, std::string("volume binning kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
        if (int rc = launch_voldzone(a, st)) return fail(ctx, NYXHIP_ERR_HIP, std::string("3-D GLDZM kernels: launch failed: ") + hipGetErrorString((hipError_t)rc));
    }
    return NYXHIP_OK;
}

} // namespace

extern "C" {

int nyxhip_voldzone_n_columns(uint32_t dmask) { return dzone_mask_ok(dmask) ? kVdzCols : -1; }

int nyxhip_voldzone_column_name(uint32_t dmask, int col, char* buf, size_t buf_len)
{
    if (!buf || buf_len == 0 || !dzone_mask_ok(dmask) || col < 0 || col >= kVdzCols) return NYXHIP_ERR_INVALID_ARG;
    snprintf(buf, buf_len, "3GLDZM_%s", kGldzmNames[col]);
    return NYXHIP_OK;
}

int nyxhip_featurize_volumes_dzones(nyxhip_ctx* ctx, const nyxhip_batch3d* b, uint32_t dmask, const nyxhip_settings* s, double* out, size_t ld)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (!b || !s || !out) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null batch / settings / out_table");
    if (!dzone_mask_ok(dmask)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad distance-zone mask: NYXHIP_VDZ_GLDZM is the bit it has");
    if (b->n_roi && (!b->px_offset || !b->inten || !b->min_inten || !b->max_inten || !b->x || !b->y || !b->z || !b->bbox_w || !b->bbox_h || !b->bbox_d))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "batch has null array pointers (px_offset, x, y, z, inten, bbox_w, bbox_h, bbox_d, min_inten, max_inten)");
    if (ld < (size_t)kVdzCols) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    if (b->n_roi > 0x7FFFFFFFull) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "too many ROIs in one batch");
    if (b->memory != NYXHIP_MEM_DEVICE && b->memory != NYXHIP_MEM_HOST) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad batch->memory");
    if (!s->ibsi && (uint32_t)std::abs((long long)s->grey_depth) > kVzLevelCap)
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, kCapText + "; |grey_depth| (coarse_gray_depth) = " + std::to_string(std::abs((long long)s->grey_depth)) + " exceeds that cap");
    return vol_run(ctx, b, true, (size_t)kVdzCols, out, ld,
                   [&](const nyxhip_batch3d& d, double* d_out, size_t d_ld, uint32_t max_px, uint32_t max_cells) {
                       return voldzone_device(ctx, d, s, d_out, d_ld, max_px, max_cells);
                   },
                   voldzone_check_status);
}

} // extern "C"
