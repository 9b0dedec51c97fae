// nyxhip_voldzone.hip -- the volume distance-zone entries of include/nyxhip.h: the column catalogue of the distance-zone mask
// (nyxhip_voldzone_n_columns, nyxhip_voldzone_column_name) and nyxhip_featurize_volumes_dzones: its cap check, then the host path of
// vol_host.h (checks, staging, the largest box sides of the batch -- they size the tables and the grids --, chunks, binned boxes); here
// the filling of VoldzoneArgs, the regions of the workspace and the launches of roi_voldzone.hip.
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
const VolTexts kTexts = {
    "volume distance zones", "settings", kVolArraysAll,
    "volume distance zones: a level is a table row and a byte of the binned box, up to NYXHIP_VOLDZONE_MAX_LEVELS = " + std::to_string(kVzLevelCap) + " levels",
    "IBSI mode, or coarse_gray_depth = 0", "", "a device loop reached the bound derived from its box (a label chase or a zone metric)", true};

// the ROIs of a device-resident batch -> d_out [n_roi x ld] (device), in chunks whose workspace fits the budget; enqueued on the stream
int voldzone_device(nyxhip_ctx* ctx, const nyxhip_batch3d& b, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px, uint32_t max_cells,
                    const VolSides& sides)
{
    hipStream_t st = ctx->stream();
    VoldzoneArgs a;
    memset(&a, 0, sizeof(a));
    a.px_offset = b.px_offset;
    a.bbox_w = b.bbox_w; a.bbox_h = b.bbox_h; a.bbox_d = b.bbox_d; a.vmin = b.min_inten; a.vmax = b.max_inten;
    a.soft_nan = s->soft_nan; a.out = d_out; a.ld = ld;
    a.status = ctx->d_status.as<int>();
    // (the tables are sized by the largest min(w, h) of the batch, the grids by its largest sides)
    const size_t per_roi = voldzone_layout(a, s, max_cells, sides);
    uint64_t chunk = 0;
    if (int rc = vol_plan_chunks(ctx, kTexts, b, per_roi, chunk)) return rc;
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
        if (int rc = vol_bin(ctx, b, a.roi0, a.n_roi, boxes, a.box_stride, a.g, max_px, max_cells)) return rc;
        if (int rc = launched(ctx, launch_voldzone(a, st), "3-D GLDZM kernels")) return rc;
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
    if (int rc = vol_entry_checks(ctx, kTexts, b, s != nullptr, out, dzone_mask_ok(dmask) ? nullptr : "bad distance-zone mask: NYXHIP_VDZ_GLDZM is the bit it has", true, false,
                                  (size_t)kVdzCols, ld))
        return rc;
    if (!s->ibsi && (uint32_t)std::abs((long long)s->grey_depth) > kVzLevelCap)
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, kTexts.cap + "; |grey_depth| (coarse_gray_depth) = " + std::to_string(std::abs((long long)s->grey_depth)) + " exceeds that cap");
    return vol_run(ctx, kTexts, b, true, (size_t)kVdzCols, out, ld,
                   [&](const nyxhip_batch3d& d, double* d_out, size_t d_ld, uint32_t max_px, uint32_t max_cells, const VolSides& sides) {
                       return voldzone_device(ctx, d, s, d_out, d_ld, max_px, max_cells, sides);
                   });
}

} // extern "C"
