// nyxhip_volshape.hip -- the volume shape entries of include/nyxhip.h: the column catalogue of the shape mask (nyxhip_vshape_n_columns,
// nyxhip_vshape_column_name) and nyxhip_featurize_volumes_shape: the host path of vol_host.h (checks, staging, the largest box sides of
// the batch -- they size the row tables and the hull's workspace --, chunks); here the filling of VolshapeArgs, the regions of the
// workspace and the launches of roi_volshape.hip.  The class bins nothing: no grey depth, no level cap.
#include "nyxhip_ctx.h"
#include "vol_host.h"
#include "roi_vol.h"
#include "roi_volshape.h"

using namespace nyxhip;

namespace {

// Feature3D order (featureset.h:678-693); the user-facing names are these behind a "3" (featureset.cpp:712-725)
const char* const kShapeNames[kVshCols] = {"AREA", "AREA_2_VOLUME", "COMPACTNESS1", "COMPACTNESS2", "MESH_VOLUME", "SPHERICAL_DISPROPORTION", "SPHERICITY",
                                           "VOLUME_CONVEXHULL", "VOXEL_VOLUME", "MAJOR_AXIS_LEN", "MINOR_AXIS_LEN", "LEAST_AXIS_LEN", "ELONGATION", "FLATNESS"};

bool shape_mask_ok(uint32_t m) { return m == (uint32_t)NYXHIP_VSHAPE_MORPHOLOGY; }
const VolTexts kTexts = {
    "volume shape", "settings", kVolArraysAll, "", "", "",
    "a loop of the hull reached the bound derived from its candidate count, or an edge of the hull was left without its twin", true};

// the ROIs of a device-resident batch -> d_out [n_roi x ld] (device), in chunks whose workspace fits the budget; enqueued on the stream
int volshape_device(nyxhip_ctx* ctx, const nyxhip_batch3d& b, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px, uint32_t max_cells,
                    const VolSides& sides)
{
    hipStream_t st = ctx->stream();
    VolshapeArgs a;
    memset(&a, 0, sizeof(a));
    a.px_offset = b.px_offset; a.x = b.x; a.y = b.y; a.z = b.z; a.inten = b.inten;
    a.bbox_w = b.bbox_w; a.bbox_h = b.bbox_h; a.bbox_d = b.bbox_d;
    a.soft_nan = s->soft_nan; a.out = d_out; a.ld = ld;
    a.status = ctx->d_status.as<int>();
    const VolshapeLayout L = volshape_layout(a, max_px, max_cells, sides);
    uint64_t chunk = 0;
    if (int rc = vol_plan_chunks(ctx, kTexts, b, L.per_roi, chunk)) return rc;
    // the workspace: what a chunk starts from zeroed (heads, row extremes, occupancy boxes: one memset), then chains, candidates, the
    // visited sets and the edge stacks
    char* const base = ctx->d_vol.as<char>();
    a.head = (unsigned long long*)base;
    a.row_lo = (uint32_t*)(a.head + chunk * kVshHead);
    a.row_hi = a.row_lo + chunk * a.row_stride;
    a.occ = (unsigned char*)(a.row_hi + chunk * a.row_stride);
    a.chain = (uint32_t*)(a.occ + chunk * a.occ_stride);
    a.cand = (unsigned long long*)(a.chain + chunk * 2 * a.row_stride);
    a.visited = a.cand + chunk * a.cand_stride;
    a.stack = a.visited + chunk * a.visited_stride;
    for (uint64_t r0 = 0; r0 < b.n_roi; r0 += chunk) {
        a.roi0 = r0; a.n_roi = std::min<uint64_t>(chunk, b.n_roi - r0);
        HIP_TRY(ctx, hipMemsetAsync(base, 0, (size_t)chunk * L.zeroed, st));
        if (int rc = launched(ctx, launch_volshape(a, st), "3-D shape kernels")) return rc;
    }
    return NYXHIP_OK;
}

} // namespace

extern "C" {

int nyxhip_vshape_n_columns(uint32_t smask) { return shape_mask_ok(smask) ? kVshCols : -1; }

int nyxhip_vshape_column_name(uint32_t smask, int col, char* buf, size_t buf_len)
{
    if (!buf || buf_len == 0 || !shape_mask_ok(smask) || col < 0 || col >= kVshCols) return NYXHIP_ERR_INVALID_ARG;
    snprintf(buf, buf_len, "3%s", kShapeNames[col]);
    return NYXHIP_OK;
}

int nyxhip_featurize_volumes_shape(nyxhip_ctx* ctx, const nyxhip_batch3d* b, uint32_t smask, const nyxhip_settings* s, double* out, size_t ld)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (int rc = vol_entry_checks(ctx, kTexts, b, s != nullptr, out, shape_mask_ok(smask) ? nullptr : "bad shape mask: NYXHIP_VSHAPE_MORPHOLOGY is the bit it has", true, false,
                                  (size_t)kVshCols, ld))
        return rc;
    return vol_run(ctx, kTexts, b, true, (size_t)kVshCols, out, ld,
                   [&](const nyxhip_batch3d& d, double* d_out, size_t d_ld, uint32_t max_px, uint32_t max_cells, const VolSides& sides) {
                       return volshape_device(ctx, d, s, d_out, d_ld, max_px, max_cells, sides);
                   });
}

} // extern "C"
