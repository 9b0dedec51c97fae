// nyxhip_voltex.hip -- the volume texture entries of include/nyxhip.h: the column catalogue of the texture mask (nyxhip_voltex_n_columns,
// nyxhip_voltex_column_name) and nyxhip_featurize_volumes_tex: checks, then (vol_host.h) the staging of a host batch; here the chunks of
// ROIs under the device budget, the binned boxes (launch_vol_bin of roi_vol.hip; NGLDM's own form) and the launches of roi_voltex.hip.
#include "nyxhip_ctx.h"
#include "vol_host.h"
#include "roi_voltex.h"

using namespace nyxhip;

namespace {

// Feature3D order under the reference's user-facing names (featureset.cpp:827-840, :911-935)
const char* const kGldmNames[kVtGldmCols] = {"SDE", "LDE", "GLN", "DN", "DNN", "GLV", "DV", "DE", "LGLE", "HGLE", "SDLGLE", "SDHGLE", "LDLGLE", "LDHGLE"};
const char* const kNgldmNames[kVtNgldmCols] = {"LDE", "HDE", "LGLCE", "HGLCE", "LDLGLE", "LDHGLE", "HDLGLE", "HDHGLE", "GLNU", "GLNUN", "DCNU", "DCNUN", "DCP",
                                               "GLM", "GLV", "DCM", "DCV", "DCENT", "DCENE"};
const char* const kNgtdmNames[kVtNgtdmCols] = {"COARSENESS", "CONTRAST", "BUSYNESS", "COMPLEXITY", "STRENGTH"};

bool tex_mask_ok(uint32_t m) { return m != 0 && (m & ~(uint32_t)NYXHIP_VTEX_ALL) == 0; }
int tex_cols(uint32_t m)
{
    return ((m & NYXHIP_VTEX_GLDM) ? kVtGldmCols : 0) + ((m & NYXHIP_VTEX_NGLDM) ? kVtNgldmCols : 0) + ((m & NYXHIP_VTEX_NGTDM) ? kVtNgtdmCols : 0);
}
size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
const std::string kCapText = "volume textures: the level tables live in LDS up to NYXHIP_VOLTEX_MAX_LEVELS = " + std::to_string(kVtLevelCap) + " levels";

int voltex_check_status(nyxhip_ctx* ctx)
{
    const int rc = check_status(ctx);
    if (rc == NYXHIP_ERR_UNSUPPORTED)
        return fail(ctx, rc, kCapText + ", and an ROI has a larger intensity (IBSI mode, or gldm_grey_depth / ngtdm_grey_depth = 0: the levels are the intensities)");
    if (rc == NYXHIP_ERR_ROI_TOO_LARGE)
        return fail(ctx, rc, "volume textures: an ROI exceeds the stated extrema, a box side of " + std::to_string(kVolMaxSide) + " or " + std::to_string(kVolMaxCells) + " cells");
    if (rc == NYXHIP_ERR_INVALID_ARG) return fail(ctx, rc, "volume textures: a voxel lies outside its box");
    return rc;
}

// the ROIs of a device-resident batch -> d_out [n_roi x ld] (device), in chunks whose workspace fits the budget; enqueued on the stream
int voltex_device(nyxhip_ctx* ctx, const nyxhip_batch3d& b, uint32_t tmask, const nyxhip_settings* s, const nyxhip_voltex_settings* t, double* d_out, size_t ld,
                  uint32_t max_px, uint32_t max_cells)
{
    hipStream_t st = ctx->stream();
    const bool gldm = (tmask & NYXHIP_VTEX_GLDM) != 0, ngldm = (tmask & NYXHIP_VTEX_NGLDM) != 0, ngtdm = (tmask & NYXHIP_VTEX_NGTDM) != 0;
    const bool tsweep = ngtdm && t->ngtdm_radius > 0;      // (radius 0 needs neither a box nor a table)
    VoltexArgs a;
    memset(&a, 0, sizeof(a));
    a.px_offset = b.px_offset; a.x = b.x; a.y = b.y; a.z = b.z; a.inten = b.inten;
    a.bbox_w = b.bbox_w; a.bbox_h = b.bbox_h; a.bbox_d = b.bbox_d; a.vmin = b.min_inten; a.vmax = b.max_inten;
    a.ibsi = s->ibsi ? 1 : 0;
    a.g_gldm = s->ibsi ? 0 : t->gldm_grey_depth;           // 3d_gldm.cpp:93-95
    a.g_ngtdm = s->ibsi ? 0 : t->ngtdm_grey_depth;         // 3d_ngtdm.cpp:195-197
    a.ngldm_levels = (uint32_t)s->grey_depth;
    a.radius = t->ngtdm_radius;
    a.soft_nan = s->soft_nan; a.out = d_out; a.ld = ld;
    a.col_gldm = gldm ? 0 : -1;
    a.col_ngldm = ngldm ? (gldm ? kVtGldmCols : 0) : -1;
    a.col_ngtdm = ngtdm ? (gldm ? kVtGldmCols : 0) + (ngldm ? kVtNgldmCols : 0) : -1;
    a.status = ctx->d_status.as<int>();
    a.max_cells = max_cells ? max_cells : 1u;
    a.box_stride = al256(a.max_cells);
    // GLDM and NGTDM share a box when they share a greyInfo
    const bool share = gldm && tsweep && a.g_gldm == a.g_ngtdm;
    const int nbox = (gldm ? 1 : 0) + (ngldm ? 1 : 0) + (tsweep && !share ? 1 : 0);
    a.tab_stride[VT_GLDM] = gldm ? al256(4 * (size_t)kVtGldmWords) >> 2 : 0;
    a.tab_stride[VT_NGLDM] = ngldm ? al256(4 * (size_t)kVtNgldmWords) >> 2 : 0;
    a.tab_stride[VT_NGTDM] = tsweep ? al256(4 * (size_t)vt_ngtdm_words(a.radius)) >> 2 : 0;
    const size_t tab_words = a.tab_stride[0] + a.tab_stride[1] + a.tab_stride[2];
    const size_t per_roi = (size_t)nbox * a.box_stride + 4 * tab_words;
    uint64_t chunk = std::min<uint64_t>(65535, b.n_roi);   // (a grid dimension counts the ROIs of a chunk)
    if (per_roi) {
        size_t budget = 0;
        if (int rc = vol_budget(ctx, &b, ctx->d_vol.bytes, budget)) return rc;
        if (per_roi > budget)
            return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "volume textures: the workspace of one ROI (" + std::to_string(per_roi) + " bytes) does not fit max_device_bytes");
        chunk = std::min<uint64_t>(budget / per_roi, chunk);
        HIP_TRY(ctx, ctx->d_vol.reserve((size_t)chunk * per_roi, st));
    }
    // the workspace: the tables of the chunk (one memset), then the boxes
    char* const base = ctx->d_vol.as<char>();
    a.tab[VT_GLDM] = (uint32_t*)base;
    a.tab[VT_NGLDM] = a.tab[VT_GLDM] + chunk * a.tab_stride[VT_GLDM];
    a.tab[VT_NGTDM] = a.tab[VT_NGLDM] + chunk * a.tab_stride[VT_NGLDM];
    unsigned char* bx = (unsigned char*)base + 4 * chunk * tab_words;
    if (gldm) { a.box[VT_GLDM] = bx; bx += chunk * a.box_stride; }
    if (ngldm) { a.box[VT_NGLDM] = bx; bx += chunk * a.box_stride; }
    if (tsweep) a.box[VT_NGTDM] = share ? a.box[VT_GLDM] : bx;
    auto bin = [&](unsigned char* boxes, int grey_info) -> int {   // vol_bin_kernel: bin_intensities_3d with the class's greyInfo
        VolArgs v;
        memset(&v, 0, sizeof(v));
        v.roi0 = a.roi0; v.n_roi = a.n_roi; v.px_offset = a.px_offset; v.x = a.x; v.y = a.y; v.z = a.z; v.inten = a.inten;
        v.bbox_w = a.bbox_w; v.bbox_h = a.bbox_h; v.bbox_d = a.bbox_d; v.vmin = a.vmin; v.vmax = a.vmax;
        v.grey_info = grey_info; v.status = a.status; v.boxes = boxes; v.box_stride = a.box_stride;
        v.max_cells = a.max_cells; v.max_px = max_px ? max_px : 1u;
        HIP_TRY(ctx, hipMemsetAsync(boxes, vol_background_level(grey_info), (size_t)a.n_roi * a.box_stride, st));
        if (int rc = launch_vol_bin(v, st)) return fail(ctx, NYXHIP_ERR_HIP, std::string("volume binning kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
        return NYXHIP_OK;
    };
    auto launched = [&](int rc, const char* what) -> int {
        return rc ? fail(ctx, NYXHIP_ERR_HIP, std::string(what) + ": launch failed: " + hipGetErrorString((hipError_t)rc)) : NYXHIP_OK;
    };
    for (uint64_t r0 = 0; r0 < b.n_roi; r0 += chunk) {
        a.roi0 = r0; a.n_roi = std::min<uint64_t>(chunk, b.n_roi - r0);
        if (tab_words) HIP_TRY(ctx, hipMemsetAsync(base, 0, 4 * (size_t)chunk * tab_words, st));
        if (gldm) {
            if (int rc = bin(a.box[VT_GLDM], a.g_gldm)) return rc;
            if (int rc = launched(launch_voltex_sweep(a, VT_GLDM, st), "3-D GLDM sweep")) return rc;
        }
        if (ngldm) {
            HIP_TRY(ctx, hipMemsetAsync(a.box[VT_NGLDM], 0, (size_t)a.n_roi * a.box_stride, st));
            if (int rc = launched(launch_voltex_bin_ngldm(a, max_px ? max_px : 1u, st), "3-D NGLDM binning kernel")) return rc;
            if (int rc = launched(launch_voltex_sweep(a, VT_NGLDM, st), "3-D NGLDM sweep")) return rc;
        }
        if (tsweep) {
            if (!share)
                if (int rc = bin(a.box[VT_NGTDM], a.g_ngtdm)) return rc;
            if (int rc = launched(launch_voltex_sweep(a, VT_NGTDM, st), "3-D NGTDM sweep")) return rc;
        } else if (ngtdm) {
            if (int rc = launched(launch_voltex_ngtdm_r0(a, st), "3-D NGTDM radius-0 kernel")) return rc;
        }
        if (int rc = launched(launch_voltex_close(a, st), "volume texture closing")) return rc;
    }
    return NYXHIP_OK;
}

} // namespace

extern "C" {

int nyxhip_voltex_n_columns(uint32_t tmask) { return tex_mask_ok(tmask) ? tex_cols(tmask) : -1; }

int nyxhip_voltex_column_name(uint32_t tmask, int col, char* buf, size_t buf_len)
{
    if (!buf || buf_len == 0 || !tex_mask_ok(tmask) || col < 0 || col >= tex_cols(tmask)) return NYXHIP_ERR_INVALID_ARG;
    if (tmask & NYXHIP_VTEX_GLDM) {
        if (col < kVtGldmCols) { snprintf(buf, buf_len, "3GLDM_%s", kGldmNames[col]); return NYXHIP_OK; }
        col -= kVtGldmCols;
    }
    if (tmask & NYXHIP_VTEX_NGLDM) {
        if (col < kVtNgldmCols) { snprintf(buf, buf_len, "3NGLDM_%s", kNgldmNames[col]); return NYXHIP_OK; }
        col -= kVtNgldmCols;
    }
    snprintf(buf, buf_len, "3NGTDM_%s", kNgtdmNames[col]);
    return NYXHIP_OK;
}

int nyxhip_featurize_volumes_tex(nyxhip_ctx* ctx, const nyxhip_batch3d* b, uint32_t tmask, const nyxhip_settings* s, const nyxhip_voltex_settings* t,
                                 double* out, size_t ld)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (!b || !s || !t || !out) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null batch / settings / texture settings / out_table");
    if (!tex_mask_ok(tmask))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad texture mask: NYXHIP_VTEX_GLDM | NYXHIP_VTEX_NGLDM | NYXHIP_VTEX_NGTDM are the bits it has");
    if (b->n_roi && (!b->px_offset || !b->inten || !b->min_inten || !b->max_inten || !b->x || !b->y || !b->z || !b->bbox_w || !b->bbox_h || !b->bbox_d))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "batch has null array pointers (px_offset, x, y, z, inten, bbox_w, bbox_h, bbox_d, min_inten, max_inten)");
    const size_t ncol = (size_t)tex_cols(tmask);
    if (ld < ncol) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    if (b->n_roi > 0x7FFFFFFFull) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "too many ROIs in one batch");
    if (b->memory != NYXHIP_MEM_DEVICE && b->memory != NYXHIP_MEM_HOST) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad batch->memory");
    auto over = [&](const char* name, long long v) {
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, kCapText + "; " + name + " = " + std::to_string(v) + " exceeds that cap");
    };
    if (tmask & NYXHIP_VTEX_NGTDM) {
        if (t->ngtdm_radius < 0 || t->ngtdm_radius > kVtMaxRadius)
            return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "volume textures: ngtdm_radius = " + std::to_string(t->ngtdm_radius) + " is outside 0 .. NYXHIP_VOLTEX_MAX_RADIUS = " +
                                                         std::to_string(kVtMaxRadius));
        if (!s->ibsi && t->ngtdm_radius > 0 && (uint32_t)abs(t->ngtdm_grey_depth) > kVtLevelCap) return over("|ngtdm_grey_depth|", abs(t->ngtdm_grey_depth));
    }
    if ((tmask & NYXHIP_VTEX_GLDM) && !s->ibsi && (uint32_t)abs(t->gldm_grey_depth) > kVtLevelCap) return over("|gldm_grey_depth|", abs(t->gldm_grey_depth));
    if ((tmask & NYXHIP_VTEX_NGLDM) && !s->ibsi && (uint32_t)s->grey_depth > kVtLevelCap) return over("grey_depth (read as unsigned by the NGLDM class)", (uint32_t)s->grey_depth);
    return vol_run(ctx, b, true, ncol, out, ld,
                   [&](const nyxhip_batch3d& d, double* d_out, size_t d_ld, uint32_t max_px, uint32_t max_cells) {
                       return voltex_device(ctx, d, tmask, s, t, d_out, d_ld, max_px, max_cells);
                   },
                   voltex_check_status);
}

} // extern "C"
