// nyxhip_hexpoly.hip -- the hexagonality / polygonality entries of include/nyxhip.h: column names, the launches over a device-resident
// batch (hexpoly_device: the contour chain ONCE, its three readers into one scratch table, the closing kernel), and nyxhip_hexpoly_batch.
// The tile entry (nyxhip_hexpoly_tiles) lives with the tile path in nyxhip_tiles.hip.
#include "nyxhip_ctx.h"

using namespace nyxhip;

namespace nyxhip {

static const char* const kHexpolyNames[kHexpolyCols] = {"POLYGONALITY_AVE", "HEXAGONALITY_AVE", "HEXAGONALITY_STDDEV"};

int hexpoly_device(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* d_ox, const uint32_t* d_oy, const uint64_t* d_image_offset, uint64_t n_images,
                   const uint32_t* d_image_id, int32_t pixel_distance, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px,
                   uint32_t max_area, uint32_t max_side)
{
    hipStream_t st = ctx->stream();
    const uint64_t n = b->n_roi;
    if (n == 0) return NYXHIP_OK;
    if (max_px == 0 || max_area == 0 || max_side == 0)                        // a device batch without stated extrema: derive them
        if (int erc = derive_batch_extrema(ctx, b, &max_px, &max_area, &max_side)) return erc;
    if (!ctx->d_hexpoly_tan) {
        // the class's only transcendental, as the reference evaluates it (hexagonality_polygonality.cpp:51-52): the host's libm
        double host_tan[kHexpolyTanCap + 1] = {0.0, 0.0, 0.0};
        for (int k = 3; k <= kHexpolyTanCap; k++) host_tan[k] = std::tan(M_PI / (double)k);
        HIP_TRY(ctx, ctx->d_hexpoly_tan.reserve(sizeof(host_tan), nullptr));
        if (hipError_t e = hipMemcpy(ctx->d_hexpoly_tan.p, host_tan, sizeof(host_tan), hipMemcpyHostToDevice); e != hipSuccess) {
            ctx->d_hexpoly_tan.release();
            return fail(ctx, NYXHIP_ERR_HIP, std::string("tangent table upload: ") + hipGetErrorString(e));
        }
    }
    const size_t scratch = sizeof(double) * (size_t)kHexpolyInLd * n;
    HIP_TRY(ctx, ctx->d_hexpoly.reserve(scratch, st, scratch + scratch / 8));
    double* const tab = ctx->d_hexpoly.as<double>();
    // ---- the Feret columns (pixel clouds, no contour) and the contour chain, once, no reader: one call of the families' launcher -------
    MomArgs m;
    {
        OriginScope origins(ctx, d_ox, d_oy);
        if (int crc = launch_contour_families(ctx, b, NYXHIP_FAM_FERET, s, tab + kHexpolyInFeret, kHexpolyInLd, max_px, max_area, max_side, false, &m))
            return crc;
    }
    // ---- the chain's two readers: NUM_NEIGHBORS | PERIMETER and CONVEX_HULL_AREA ---------------------------------------------------------
    if (int nrc = neighbors_from_contours(ctx, b, d_ox, d_oy, d_image_offset, n_images, d_image_id, pixel_distance, m, tab + kHexpolyInNeighbors, kHexpolyInLd))
        return nrc;
    if (int mrc = morph_from_contours(ctx, b, d_ox, d_oy, NYXHIP_MORPH_CONTOUR | NYXHIP_MORPH_HULL, m, tab + kHexpolyInMorph, kHexpolyInLd, max_area, max_side))
        return mrc;
    // ---- the closing formula, a lane per ROI ---------------------------------------------------------------------------------------------
    HexArgs a;
    memset(&a, 0, sizeof(a));
    a.n_roi = n;
    a.px_offset = b->px_offset; a.n_contour = m.n_contour;
    a.in = tab; a.tan_tab = ctx->d_hexpoly_tan.as<double>();
    a.out = d_out; a.ld = ld;
    if (int rc = launch_roi_hexpoly(a, st))
        return fail(ctx, NYXHIP_ERR_HIP, std::string("hexagonality / polygonality kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
    return NYXHIP_OK;
}

} // namespace nyxhip

extern "C" {

int nyxhip_hexpoly_column_name(int col, char* buf, size_t buf_len)
{
    if (!buf || buf_len == 0 || col < 0 || col >= kHexpolyCols) return NYXHIP_ERR_INVALID_ARG;
    snprintf(buf, buf_len, "%s", kHexpolyNames[col]);
    return NYXHIP_OK;
}

int nyxhip_hexpoly_batch(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y, const uint64_t* image_offset,
                         uint64_t n_images, int32_t pixel_distance, const nyxhip_settings* s, double* out, size_t ld)
{
    return image_batch_entry(ctx, b, origin_x, origin_y, image_offset, n_images, pixel_distance, s, out, ld, kHexpolyCols, hexpoly_device);
}

} // extern "C"
