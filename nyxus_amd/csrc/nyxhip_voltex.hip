// nyxhip_voltex.hip -- the volume texture entries of include/nyxhip.h: the column catalogue of the texture mask (nyxhip_voltex_n_columns,
// nyxhip_voltex_column_name) and nyxhip_featurize_volumes_tex: its cap checks, then the host path of vol_host.h (checks, staging, chunks,
// binned boxes); here the filling of VoltexArgs, the regions of the workspace, NGLDM's own binning and the launches of roi_voltex.hip.
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
const VolTexts kTexts = {
    "volume textures", "settings / texture settings", kVolArraysAll,
    "volume textures: the level tables live in LDS up to NYXHIP_VOLTEX_MAX_LEVELS = " + std::to_string(kVtLevelCap) + " levels",
    "IBSI mode, or gldm_grey_depth / ngtdm_grey_depth = 0", "", nullptr, false};

// the ROIs of a device-resident batch -> d_out [n_roi x ld] (device), in chunks whose workspace fits the budget; enqueued on the stream
int voltex_device(nyxhip_ctx* ctx, const nyxhip_batch3d& b, uint32_t tmask, const nyxhip_settings* s, const nyxhip_voltex_settings* t, double* d_out, size_t ld,
                  uint32_t max_px, uint32_t max_cells)
{
    hipStream_t st = ctx->stream();
    const bool gldm = (tmask & NYXHIP_VTEX_GLDM) != 0, ngldm = (tmask & NYXHIP_VTEX_NGLDM) != 0, ngtdm = (tmask & NYXHIP_VTEX_NGTDM) != 0;
    VoltexArgs a;
    memset(&a, 0, sizeof(a));
    a.px_offset = b.px_offset; a.x = b.x; a.y = b.y; a.z = b.z; a.inten = b.inten;
    a.bbox_w = b.bbox_w; a.bbox_h = b.bbox_h; a.bbox_d = b.bbox_d; a.vmin = b.min_inten; a.vmax = b.max_inten;
    a.ibsi = s->ibsi ? 1 : 0;
    a.ngldm_levels = (uint32_t)s->grey_depth;
    a.soft_nan = s->soft_nan; a.out = d_out; a.ld = ld;
    a.col_gldm = gldm ? 0 : -1;
    a.col_ngldm = ngldm ? (gldm ? kVtGldmCols : 0) : -1;
    a.col_ngtdm = ngtdm ? (gldm ? kVtGldmCols : 0) + (ngldm ? kVtNgldmCols : 0) : -1;
    a.status = ctx->d_status.as<int>();
    const VoltexLayout L = voltex_layout(a, tmask, s, t, max_cells);
    const bool tsweep = L.tsweep, share = L.share;         // (NGTDM at radius 0 needs neither a box nor a table)
    const size_t tab_words = L.tab_words;
    uint64_t chunk = 0;
    if (int rc = vol_plan_chunks(ctx, kTexts, b, L.per_roi, chunk)) return rc;
    // the workspace: the tables of the chunk (one memset), then the boxes
    char* const base = ctx->d_vol.as<char>();
    a.tab[VT_GLDM] = (uint32_t*)base;
    a.tab[VT_NGLDM] = a.tab[VT_GLDM] + chunk * a.tab_stride[VT_GLDM];
    a.tab[VT_NGTDM] = a.tab[VT_NGLDM] + chunk * a.tab_stride[VT_NGLDM];
    unsigned char* bx = (unsigned char*)base + 4 * chunk * tab_words;
    if (gldm) { a.box[VT_GLDM] = bx; bx += chunk * a.box_stride; }
    if (ngldm) { a.box[VT_NGLDM] = bx; bx += chunk * a.box_stride; }
    if (tsweep) a.box[VT_NGTDM] = share ? a.box[VT_GLDM] : bx;
    auto bin = [&](unsigned char* boxes, int grey_info) { return vol_bin(ctx, b, a.roi0, a.n_roi, boxes, a.box_stride, grey_info, max_px, max_cells); };
    for (uint64_t r0 = 0; r0 < b.n_roi; r0 += chunk) {
        a.roi0 = r0; a.n_roi = std::min<uint64_t>(chunk, b.n_roi - r0);
        if (tab_words) HIP_TRY(ctx, hipMemsetAsync(base, 0, 4 * (size_t)chunk * tab_words, st));
        if (gldm) {
            if (int rc = bin(a.box[VT_GLDM], a.g_gldm)) return rc;
            if (int rc = launched(ctx, launch_voltex_sweep(a, VT_GLDM, st), "3-D GLDM sweep")) return rc;
        }
        if (ngldm) {
            HIP_TRY(ctx, hipMemsetAsync(a.box[VT_NGLDM], 0, (size_t)a.n_roi * a.box_stride, st));
            if (int rc = launched(ctx, launch_voltex_bin_ngldm(a, max_px ? max_px : 1u, st), "3-D NGLDM binning kernel")) return rc;
            if (int rc = launched(ctx, launch_voltex_sweep(a, VT_NGLDM, st), "3-D NGLDM sweep")) return rc;
        }
        if (tsweep) {
            if (!share)
                if (int rc = bin(a.box[VT_NGTDM], a.g_ngtdm)) return rc;
            if (int rc = launched(ctx, launch_voltex_sweep(a, VT_NGTDM, st), "3-D NGTDM sweep")) return rc;
        } else if (ngtdm) {
            if (int rc = launched(ctx, launch_voltex_ngtdm_r0(a, st), "3-D NGTDM radius-0 kernel")) return rc;
        }
        if (int rc = launched(ctx, launch_voltex_close(a, st), "volume texture closing")) return rc;
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
    const size_t ncol = (size_t)tex_cols(tmask);
    if (int rc = vol_entry_checks(ctx, kTexts, b, s && t, out,
                                  tex_mask_ok(tmask) ? nullptr : "bad texture mask: NYXHIP_VTEX_GLDM | NYXHIP_VTEX_NGLDM | NYXHIP_VTEX_NGTDM are the bits it has", true, false,
                                  ncol, ld))
        return rc;
    auto over = [&](const char* name, long long v) {
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, kTexts.cap + "; " + name + " = " + std::to_string(v) + " exceeds that cap");
    };
    if (tmask & NYXHIP_VTEX_NGTDM) {
        if (t->ngtdm_radius < 0 || t->ngtdm_radius > kVtMaxRadius)
            return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "volume textures: ngtdm_radius = " + std::to_string(t->ngtdm_radius) + " is outside 0 .. NYXHIP_VOLTEX_MAX_RADIUS = " +
                                                         std::to_string(kVtMaxRadius));
        if (!s->ibsi && t->ngtdm_radius > 0 && (uint32_t)abs(t->ngtdm_grey_depth) > kVtLevelCap) return over("|ngtdm_grey_depth|", abs(t->ngtdm_grey_depth));
    }
    if ((tmask & NYXHIP_VTEX_GLDM) && !s->ibsi && (uint32_t)abs(t->gldm_grey_depth) > kVtLevelCap) return over("|gldm_grey_depth|", abs(t->gldm_grey_depth));
    if ((tmask & NYXHIP_VTEX_NGLDM) && !s->ibsi && (uint32_t)s->grey_depth > kVtLevelCap) return over("grey_depth (read as unsigned by the NGLDM class)", (uint32_t)s->grey_depth);
    return vol_run(ctx, kTexts, b, true, ncol, out, ld,
                   [&](const nyxhip_batch3d& d, double* d_out, size_t d_ld, uint32_t max_px, uint32_t max_cells, const VolSides&) {
                       return voltex_device(ctx, d, tmask, s, t, d_out, d_ld, max_px, max_cells);
                   });
}

} // extern "C"
