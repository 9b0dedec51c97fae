// nyxhip_volzone.hip -- the volume zone entries of include/nyxhip.h: the column catalogue of the zone mask (nyxhip_volzone_n_columns,
// nyxhip_volzone_column_name) and nyxhip_featurize_volumes_zones: its cap checks, then the host path of vol_host.h (checks, staging, the
// largest box sides of the batch -- they size the run tables --, chunks, binned boxes); here the filling of VolzoneArgs, the regions of
// the workspace and the launches of roi_volzone.hip.
#include "nyxhip_ctx.h"
#include "vol_host.h"
#include "roi_vol.h"
#include "roi_volzone.h"

using namespace nyxhip;

namespace {

// Feature3D order under the reference's user-facing names (featureset.cpp:861-909)
const char* const kGlrlmNames[kVzGlrlmCodes] = {"SRE", "LRE", "GLN", "GLNN", "RLN", "RLNN", "RP", "GLV", "RV", "RE", "LGLRE", "HGLRE", "SRLGLE", "SRHGLE", "LRLGLE", "LRHGLE"};
const char* const kGlszmNames[kVzGlszmCols] = {"SAE", "LAE", "GLN", "GLNN", "SZN", "SZNN", "ZP", "GLV", "ZV", "ZE", "LGLZE", "HGLZE", "SALGLE", "SAHGLE", "LALGLE", "LAHGLE"};

bool zone_mask_ok(uint32_t m) { return m != 0 && (m & ~(uint32_t)NYXHIP_VZONE_ALL) == 0; }
int zone_cols(uint32_t m) { return ((m & NYXHIP_VZONE_GLRLM) ? kVzGlrlmCols : 0) + ((m & NYXHIP_VZONE_GLSZM) ? kVzGlszmCols : 0); }
const VolTexts kTexts = {
    "volume zones", "settings / zone settings", kVolArraysAll,
    "volume zones: a level is a table row and a byte of the binned box, up to NYXHIP_VOLZONE_MAX_LEVELS = " + std::to_string(kVzLevelCap) + " levels",
    "IBSI mode, or glrlm_grey_depth / glszm_grey_depth = 0", "", "a device loop reached the bound derived from its box (a label chase or a run walk)", true};

// the ROIs of a device-resident batch -> d_out [n_roi x ld] (device), in chunks whose workspace fits the budget; enqueued on the stream
int volzone_device(nyxhip_ctx* ctx, const nyxhip_batch3d& b, uint32_t zmask, const nyxhip_settings* s, const nyxhip_volzone_settings* t, double* d_out, size_t ld,
                   uint32_t max_px, uint32_t max_cells, const VolSides& sides)
{
    hipStream_t st = ctx->stream();
    const bool rl = (zmask & NYXHIP_VZONE_GLRLM) != 0, sz = (zmask & NYXHIP_VZONE_GLSZM) != 0;
    VolzoneArgs a;
    memset(&a, 0, sizeof(a));
    a.px_offset = b.px_offset; a.x = b.x; a.y = b.y; a.z = b.z; a.inten = b.inten;
    a.bbox_w = b.bbox_w; a.bbox_h = b.bbox_h; a.bbox_d = b.bbox_d; a.vmin = b.min_inten; a.vmax = b.max_inten;
    a.soft_nan = s->soft_nan; a.out = d_out; a.ld = ld;
    a.col[VZ_GLRLM] = rl ? 0 : -1;
    a.col[VZ_GLSZM] = sz ? (rl ? kVzGlrlmCols : 0) : -1;
    a.status = ctx->d_status.as<int>();
    // (the run tables are sized by the largest box sides of the batch)
    const VolzoneLayout L = volzone_layout(a, zmask, s, t, max_cells, sides);
    const bool share = L.share;
    const size_t tab_words = L.tab_words;
    uint64_t chunk = 0;
    if (int rc = vol_plan_chunks(ctx, kTexts, b, L.per_roi, chunk)) return rc;
    // the workspace: the tables of the chunk (one memset), then labels, counts, keys, boxes
    char* const base = ctx->d_vol.as<char>();
    a.rl_tab = (uint32_t*)base;
    a.sz_tab = a.rl_tab + chunk * a.rl_stride;
    a.sz_label = a.sz_tab + chunk * a.sz_stride;
    a.sz_count = a.sz_label + chunk * a.cell_stride;
    a.sz_keys = a.sz_count + chunk * a.cell_stride;
    unsigned char* bx = (unsigned char*)(a.sz_keys + 2 * chunk * a.key_stride);
    if (rl) { a.box[VZ_GLRLM] = bx; bx += chunk * a.box_stride; }
    if (sz) a.box[VZ_GLSZM] = share ? a.box[VZ_GLRLM] : bx;
    auto bin = [&](unsigned char* boxes, int grey_info) { return vol_bin(ctx, b, a.roi0, a.n_roi, boxes, a.box_stride, grey_info, max_px, max_cells); };
    for (uint64_t r0 = 0; r0 < b.n_roi; r0 += chunk) {
        a.roi0 = r0; a.n_roi = std::min<uint64_t>(chunk, b.n_roi - r0);
        HIP_TRY(ctx, hipMemsetAsync(base, 0, 4 * (size_t)chunk * tab_words, st));
        if (rl) {
            if (int rc = bin(a.box[VZ_GLRLM], a.g[VZ_GLRLM])) return rc;
            if (int rc = launched(ctx, launch_volzone_runs(a, st), "3-D GLRLM kernels")) return rc;
        }
        if (sz) {
            if (!share)
                if (int rc = bin(a.box[VZ_GLSZM], a.g[VZ_GLSZM])) return rc;
            if (int rc = launched(ctx, launch_volzone_zones(a, st), "3-D GLSZM kernels")) return rc;
        }
    }
    return NYXHIP_OK;
}

} // namespace

extern "C" {

int nyxhip_volzone_n_columns(uint32_t zmask) { return zone_mask_ok(zmask) ? zone_cols(zmask) : -1; }

int nyxhip_volzone_column_name(uint32_t zmask, int col, char* buf, size_t buf_len)
{
    if (!buf || buf_len == 0 || !zone_mask_ok(zmask) || col < 0 || col >= zone_cols(zmask)) return NYXHIP_ERR_INVALID_ARG;
    if (zmask & NYXHIP_VZONE_GLRLM) {
        if (col < kVzGlrlmCodes * kVzDirs) { snprintf(buf, buf_len, "3GLRLM_%s_%d", kGlrlmNames[col / kVzDirs], col % kVzDirs); return NYXHIP_OK; }
        col -= kVzGlrlmCodes * kVzDirs;
        if (col < kVzGlrlmCodes) { snprintf(buf, buf_len, "3GLRLM_%s_AVE", kGlrlmNames[col]); return NYXHIP_OK; }
        col -= kVzGlrlmCodes;
    }
    snprintf(buf, buf_len, "3GLSZM_%s", kGlszmNames[col]);
    return NYXHIP_OK;
}

int nyxhip_featurize_volumes_zones(nyxhip_ctx* ctx, const nyxhip_batch3d* b, uint32_t zmask, const nyxhip_settings* s, const nyxhip_volzone_settings* t,
                                   double* out, size_t ld)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    const size_t ncol = (size_t)zone_cols(zmask);
    if (int rc = vol_entry_checks(ctx, kTexts, b, s && t, out, zone_mask_ok(zmask) ? nullptr : "bad zone mask: NYXHIP_VZONE_GLRLM | NYXHIP_VZONE_GLSZM are the bits it has", true,
                                  false, ncol, ld))
        return rc;
    auto over = [&](const char* name, long long v) {
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, kTexts.cap + "; " + name + " = " + std::to_string(v) + " exceeds that cap");
    };
    if ((zmask & NYXHIP_VZONE_GLRLM) && !s->ibsi && (uint32_t)std::abs((long long)t->glrlm_grey_depth) > kVzLevelCap)
        return over("|glrlm_grey_depth|", std::abs((long long)t->glrlm_grey_depth));
    if ((zmask & NYXHIP_VZONE_GLSZM) && !s->ibsi && (uint32_t)std::abs((long long)t->glszm_grey_depth) > kVzLevelCap)
        return over("|glszm_grey_depth|", std::abs((long long)t->glszm_grey_depth));
    return vol_run(ctx, kTexts, b, true, ncol, out, ld,
                   [&](const nyxhip_batch3d& d, double* d_out, size_t d_ld, uint32_t max_px, uint32_t max_cells, const VolSides& sides) {
                       return volzone_device(ctx, d, zmask, s, t, d_out, d_ld, max_px, max_cells, sides);
                   });
}

} // extern "C"
