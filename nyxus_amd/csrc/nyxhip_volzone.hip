// nyxhip_volzone.hip -- the volume zone entries of include/nyxhip.h: the column catalogue of the zone mask (nyxhip_volzone_n_columns,
// nyxhip_volzone_column_name) and nyxhip_featurize_volumes_zones: checks, then (vol_host.h) the staging of a host batch; here the largest
// box sides of the batch (they size the run tables), the chunks of ROIs under the device budget, the binned boxes (launch_vol_bin of
// roi_vol.hip) and the launches of roi_volzone.hip.
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
size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
const std::string kCapText = "volume zones: a level is a table row and a byte of the binned box, up to NYXHIP_VOLZONE_MAX_LEVELS = " + std::to_string(kVzLevelCap) + " levels";

int volzone_check_status(nyxhip_ctx* ctx)
{
    const int rc = check_status(ctx);
    if (rc == NYXHIP_ERR_UNSUPPORTED)
        return fail(ctx, rc, kCapText + ", and an ROI has a larger intensity (IBSI mode, or glrlm_grey_depth / glszm_grey_depth = 0: the levels are the intensities)");
    if (rc == NYXHIP_ERR_ROI_TOO_LARGE)
        return fail(ctx, rc, "volume zones: an ROI exceeds the stated extrema, a box side of " + std::to_string(kVolMaxSide) + " or " + std::to_string(kVolMaxCells) + " cells");
    if (rc == NYXHIP_ERR_INVALID_ARG) return fail(ctx, rc, "volume zones: a voxel lies outside its box");
    if (rc == NYXHIP_ERR_INTERNAL) return fail(ctx, rc, "volume zones: a device loop reached the bound derived from its box (a label chase or a run walk)");
    return rc;
}

// the ROIs of a device-resident batch -> d_out [n_roi x ld] (device), in chunks whose workspace fits the budget; enqueued on the stream
int volzone_device(nyxhip_ctx* ctx, const nyxhip_batch3d& b, uint32_t zmask, const nyxhip_settings* s, const nyxhip_volzone_settings* t, double* d_out, size_t ld,
                   uint32_t max_px, uint32_t max_cells)
{
    hipStream_t st = ctx->stream();
    const bool rl = (zmask & NYXHIP_VZONE_GLRLM) != 0, sz = (zmask & NYXHIP_VZONE_GLSZM) != 0;
    VolzoneArgs a;
    memset(&a, 0, sizeof(a));
    a.px_offset = b.px_offset; a.x = b.x; a.y = b.y; a.z = b.z; a.inten = b.inten;
    a.bbox_w = b.bbox_w; a.bbox_h = b.bbox_h; a.bbox_d = b.bbox_d; a.vmin = b.min_inten; a.vmax = b.max_inten;
    a.g[VZ_GLRLM] = s->ibsi ? 0 : t->glrlm_grey_depth;     // 3d_glrlm.cpp:147-149
    a.g[VZ_GLSZM] = s->ibsi ? 0 : t->glszm_grey_depth;     // 3d_glszm.cpp:490-492
    for (int c = 0; c < 2; c++) a.rows[c] = (a.g[c] ? (uint32_t)abs(a.g[c]) : kVzLevelCap) + 1u;
    a.soft_nan = s->soft_nan; a.out = d_out; a.ld = ld;
    a.col[VZ_GLRLM] = rl ? 0 : -1;
    a.col[VZ_GLSZM] = sz ? (rl ? kVzGlrlmCols : 0) : -1;
    a.status = ctx->d_status.as<int>();
    a.max_cells = max_cells ? max_cells : 1u;
    a.box_stride = al256(a.max_cells);
    // the run tables are sized by the largest box sides of the batch: one copy of the boxes, whatever extrema are stated
    {
        const uint64_t nr = b.n_roi;
        std::vector<uint32_t> whd(3 * nr);
        HIP_TRY(ctx, hipMemcpyAsync(whd.data(), b.bbox_w, 4 * nr, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(whd.data() + nr, b.bbox_h, 4 * nr, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(whd.data() + 2 * nr, b.bbox_d, 4 * nr, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (int ax = 0; ax < 3; ax++) {
            uint32_t m = 1;
            for (uint64_t r = 0; r < nr; r++) {
                const uint32_t w = whd[r], h = whd[nr + r], d = whd[2 * nr + r];
                if (w > kVolMaxSide || h > kVolMaxSide || d > kVolMaxSide || (uint64_t)w * h * d > (uint64_t)a.max_cells) continue;   // (refused on the device)
                m = std::max(m, whd[ax * nr + r]);
            }
            a.side_max[ax] = m;
        }
    }
    const bool share = rl && sz && a.g[VZ_GLRLM] == a.g[VZ_GLSZM];
    const int nbox = (rl ? 1 : 0) + (sz ? 1 : 0) - (share ? 1 : 0);
    size_t rl_words = 0;
    if (rl) {
        rl_words = kVzRlHead;
        for (int k = 0; k < kVzDirs; k++) {
            a.rl_dir_off[k] = rl_words;
            rl_words += (size_t)a.rows[VZ_GLRLM] * vz_dir_len(kVzShifts[k][0], kVzShifts[k][1], kVzShifts[k][2], a.side_max[0], a.side_max[1], a.side_max[2]);
        }
        a.rl_stride = al256(4 * rl_words) >> 2;
    }
    if (sz) {
        a.sz_stride = al256(4 * (size_t)(kVzSzHead + a.rows[VZ_GLSZM] * kVzDenseSizes)) >> 2;
        a.cell_stride = al256(4 * (size_t)a.max_cells) >> 2;
        a.key_stride = al256(4 * ((size_t)a.max_cells / (kVzDenseSizes + 1u) + 1u)) >> 2;
    }
    const size_t tab_words = a.rl_stride + a.sz_stride;
    const size_t per_roi = (size_t)nbox * a.box_stride + 4 * (tab_words + 2 * a.cell_stride + 2 * a.key_stride);
    size_t budget = 0;
    if (int rc = vol_budget(ctx, &b, ctx->d_vol.bytes, budget)) return rc;
    if (per_roi > budget)
        return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "volume zones: the workspace of one ROI (" + std::to_string(per_roi) + " bytes) does not fit max_device_bytes");
    const uint64_t chunk = std::min<uint64_t>(budget / per_roi, std::min<uint64_t>(65535, b.n_roi));   // (a grid dimension counts the ROIs of a chunk)
    HIP_TRY(ctx, ctx->d_vol.reserve((size_t)chunk * per_roi, st));
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
        HIP_TRY(ctx, hipMemsetAsync(base, 0, 4 * (size_t)chunk * tab_words, st));
        if (rl) {
            if (int rc = bin(a.box[VZ_GLRLM], a.g[VZ_GLRLM])) return rc;
            if (int rc = launched(launch_volzone_runs(a, st), "3-D GLRLM kernels")) return rc;
        }
        if (sz) {
            if (!share)
                if (int rc = bin(a.box[VZ_GLSZM], a.g[VZ_GLSZM])) return rc;
            if (int rc = launched(launch_volzone_zones(a, st), "3-D GLSZM kernels")) return rc;
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
    if (!b || !s || !t || !out) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null batch / settings / zone settings / out_table");
    if (!zone_mask_ok(zmask)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad zone mask: NYXHIP_VZONE_GLRLM | NYXHIP_VZONE_GLSZM are the bits it has");
    if (b->n_roi && (!b->px_offset || !b->inten || !b->min_inten || !b->max_inten || !b->x || !b->y || !b->z || !b->bbox_w || !b->bbox_h || !b->bbox_d))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "batch has null array pointers (px_offset, x, y, z, inten, bbox_w, bbox_h, bbox_d, min_inten, max_inten)");
    const size_t ncol = (size_t)zone_cols(zmask);
    if (ld < ncol) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    if (b->n_roi > 0x7FFFFFFFull) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "too many ROIs in one batch");
    if (b->memory != NYXHIP_MEM_DEVICE && b->memory != NYXHIP_MEM_HOST) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad batch->memory");
    auto over = [&](const char* name, long long v) {
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, kCapText + "; " + name + " = " + std::to_string(v) + " exceeds that cap");
    };
    if ((zmask & NYXHIP_VZONE_GLRLM) && !s->ibsi && (uint32_t)std::abs((long long)t->glrlm_grey_depth) > kVzLevelCap)
        return over("|glrlm_grey_depth|", std::abs((long long)t->glrlm_grey_depth));
    if ((zmask & NYXHIP_VZONE_GLSZM) && !s->ibsi && (uint32_t)std::abs((long long)t->glszm_grey_depth) > kVzLevelCap)
        return over("|glszm_grey_depth|", std::abs((long long)t->glszm_grey_depth));
    return vol_run(ctx, b, true, ncol, out, ld,
                   [&](const nyxhip_batch3d& d, double* d_out, size_t d_ld, uint32_t max_px, uint32_t max_cells) {
                       return volzone_device(ctx, d, zmask, s, t, d_out, d_ld, max_px, max_cells);
                   },
                   volzone_check_status);
}

} // extern "C"
