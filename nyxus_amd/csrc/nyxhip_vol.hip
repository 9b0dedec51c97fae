// nyxhip_vol.hip -- the volume entries of include/nyxhip.h: the column catalogue of the volume mask (nyxhip_vol_n_columns,
// nyxhip_vol_column_name) and nyxhip_featurize_volumes: its checks and the launches of roi_vol.hip per chunk.  Defines the host path
// of vol_host.h that the four volume entry files share.
#include "nyxhip_ctx.h"
#include "vol_host.h"

using namespace nyxhip;

namespace {

// Feature3D order (featureset.h:646-676); the user-facing names are these behind a "3" (featureset.cpp:674-709)
const char* const kVolIntensityNames[kVolIntensityCols] = {
    "COV", "COVERED_IMAGE_INTENSITY_RANGE", "ENERGY", "ENTROPY", "EXCESS_KURTOSIS", "HYPERFLATNESS", "HYPERSKEWNESS", "INTEGRATED_INTENSITY",
    "INTERQUARTILE_RANGE", "KURTOSIS", "MAX", "MEAN", "MEAN_ABSOLUTE_DEVIATION", "MEDIAN", "MEDIAN_ABSOLUTE_DEVIATION", "MIN", "MODE", "P01", "P10",
    "P25", "P75", "P90", "P99", "QCOD", "RANGE", "ROBUST_MEAN", "ROBUST_MEAN_ABSOLUTE_DEVIATION", "ROOT_MEAN_SQUARED", "SKEWNESS",
    "STANDARD_DEVIATION", "STANDARD_DEVIATION_BIASED", "STANDARD_ERROR", "VARIANCE", "VARIANCE_BIASED", "UNIFORMITY", "UNIFORMITY_PIU"};
// Feature3D order (featureset.h:739-768)
const char* const kVolGlcmNames[kVolGlcmAngled] = {
    "ACOR", "ASM", "CLUPROM", "CLUSHADE", "CLUTEND", "CONTRAST", "CORRELATION", "DIFAVE", "DIFENTRO", "DIFVAR", "DIS", "ENERGY", "ENTROPY", "HOM1",
    "HOM2", "ID", "IDN", "IDM", "IDMN", "INFOMEAS1", "INFOMEAS2", "IV", "JAVE", "JE", "JMAX", "JVAR", "SUMAVERAGE", "SUMENTROPY", "SUMVARIANCE",
    "VARIANCE"};
// Feature3D order (featureset.h:769-797)
const char* const kVolGlcmAveNames[kVolGlcmAve] = {
    "ASM", "ACOR", "CLUPROM", "CLUSHADE", "CLUTEND", "CONTRAST", "CORRELATION", "DIFAVE", "DIFENTRO", "DIFVAR", "DIS", "ENERGY", "ENTROPY", "HOM1",
    "ID", "IDN", "IDM", "IDMN", "IV", "JAVE", "JE", "INFOMEAS1", "INFOMEAS2", "VARIANCE", "JMAX", "JVAR", "SUMAVERAGE", "SUMENTROPY", "SUMVARIANCE"};

constexpr uint32_t kVolMaxHistBins = 16384;            // the bounds of the intensity histogram's bins live in LDS

bool vol_mask_ok(uint32_t m) { return m != 0 && (m & ~(uint32_t)NYXHIP_VFAM_ALL) == 0; }
int vol_cols(uint32_t m) { return ((m & NYXHIP_VFAM_INTENSITY) ? kVolIntensityCols : 0) + ((m & NYXHIP_VFAM_GLCM) ? kVolGlcmCols : 0); }

const VolTexts kTexts = {
    "volumes", "settings", "(px_offset, inten, min_inten, max_inten; for the GLCM block also x, y, z, bbox_w, bbox_h, bbox_d)",
    "volumes: the 3-D GLCM matrix lives in LDS up to " + std::to_string(kVolLevelCap) + " levels", "IBSI mode",
    ", or an intensity outside [min_inten, max_inten]", nullptr, false};

// the ROIs of a device-resident batch -> d_out [n_roi x ld] (device), in chunks whose workspace fits the budget; enqueued on the stream
int vol_device(nyxhip_ctx* ctx, const nyxhip_batch3d* b, uint32_t vmask, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px,
               uint32_t max_cells)
{
    hipStream_t st = ctx->stream();
    const bool glcm = (vmask & NYXHIP_VFAM_GLCM) != 0, inten = (vmask & NYXHIP_VFAM_INTENSITY) != 0;
    VolArgs a;
    memset(&a, 0, sizeof(a));
    a.px_offset = b->px_offset; a.x = b->x; a.y = b->y; a.z = b->z; a.inten = b->inten;
    a.bbox_w = b->bbox_w; a.bbox_h = b->bbox_h; a.bbox_d = b->bbox_d; a.vmin = b->min_inten; a.vmax = b->max_inten;
    a.slide_min = b->slide_min; a.slide_max = b->slide_max;
    a.offset = s->glcm_offset; a.symmetric = s->glcm_symmetric;
    a.n_hist = (uint32_t)abs(s->grey_depth);
    a.soft_nan = s->soft_nan; a.out = d_out; a.ld = ld;
    a.col_intensity = inten ? 0 : -1; a.col_glcm = glcm ? (inten ? kVolIntensityCols : 0) : -1;
    a.status = ctx->d_status.as<int>();
    const size_t per_roi = vol_layout(a, vmask, s, max_px, max_cells);
    a.stage_cells = (std::min(a.max_cells, kVolLdsCells) + 15u) & ~15u;
    a.ng_bound = a.grey_info ? (uint32_t)abs(a.grey_info) : kVolLevelCap;
    uint64_t chunk = 0;
    if (int rc = vol_plan_chunks(ctx, kTexts, *b, per_roi, chunk)) return rc;
    a.boxes = ctx->d_vol.as<unsigned char>();
    a.keys = (uint32_t*)(ctx->d_vol.as<char>() + (size_t)chunk * a.box_stride);
    for (uint64_t r0 = 0; r0 < b->n_roi; r0 += chunk) {
        a.roi0 = r0; a.n_roi = std::min<uint64_t>(chunk, b->n_roi - r0);
        if (glcm) {
            if (int rc = vol_bin_launch(ctx, a)) return rc;
            if (int rc = launched(ctx, launch_vol_glcm(a, st), "3-D GLCM kernel")) return rc;
        }
        if (inten)
            if (int rc = launched(ctx, launch_vol_intensity(a, st), "voxel-intensity kernel")) return rc;
    }
    return NYXHIP_OK;
}

// the budget of a call's workspace: max_device_bytes, or half of the free device memory (`held`: what the workspace buffer already holds)
int vol_budget(nyxhip_ctx* ctx, const nyxhip_batch3d& b, size_t held, size_t& budget)
{
    budget = (size_t)b.max_device_bytes;
    if (budget == 0) {
        size_t fr = 0, tot = 0;
        HIP_TRY(ctx, hipMemGetInfo(&fr, &tot));
        const int sharers = std::max(1, g_ctx_on_device[ctx->device & 63].load());
        budget = (fr + held) / 2 / (size_t)sharers;
    }
    return NYXHIP_OK;
}

// the device status of a call, in the entry's words
int vol_check_status(nyxhip_ctx* ctx, const VolTexts& tx)
{
    const int rc = check_status(ctx);
    const std::string label = std::string(tx.label) + ": ";
    if (rc == NYXHIP_ERR_UNSUPPORTED) return fail(ctx, rc, tx.cap + ", and an ROI has a larger intensity (" + tx.unbinned + ": the levels are the intensities)");
    if (rc == NYXHIP_ERR_ROI_TOO_LARGE)
        return fail(ctx, rc, label + "an ROI exceeds the stated extrema, a box side of " + std::to_string(kVolMaxSide) + " or " + std::to_string(kVolMaxCells) + " cells");
    if (rc == NYXHIP_ERR_INVALID_ARG) return fail(ctx, rc, label + "a voxel lies outside its box" + tx.outside);
    if (rc == NYXHIP_ERR_INTERNAL && tx.internal) return fail(ctx, rc, label + tx.internal);
    return rc;
}

} // namespace

namespace nyxhip {

int vol_entry_checks(nyxhip_ctx* ctx, const VolTexts& tx, const nyxhip_batch3d* b, bool have_settings, const double* out, const char* bad_mask, bool boxes,
                     bool slide_pair, size_t ncol, size_t ld)
{
    if (!b || !have_settings || !out) return fail(ctx, NYXHIP_ERR_INVALID_ARG, std::string("null batch / ") + tx.settings + " / out_table");
    if (bad_mask) return fail(ctx, NYXHIP_ERR_INVALID_ARG, bad_mask);
    if (b->n_roi && (!b->px_offset || !b->inten || !b->min_inten || !b->max_inten || (boxes && (!b->x || !b->y || !b->z || !b->bbox_w || !b->bbox_h || !b->bbox_d))))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, std::string("batch has null array pointers ") + tx.arrays);
    if (slide_pair && (b->slide_min == nullptr) != (b->slide_max == nullptr))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "slide_min and slide_max must both be given or both NULL");
    if (ld < ncol) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    if (b->n_roi > 0x7FFFFFFFull) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "too many ROIs in one batch");
    if (b->memory != NYXHIP_MEM_DEVICE && b->memory != NYXHIP_MEM_HOST) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad batch->memory");
    return NYXHIP_OK;
}

int launched(nyxhip_ctx* ctx, int rc, const char* what)
{
    return rc ? fail(ctx, NYXHIP_ERR_HIP, std::string(what) + ": launch failed: " + hipGetErrorString((hipError_t)rc)) : NYXHIP_OK;
}

int vol_plan_chunks(nyxhip_ctx* ctx, const VolTexts& tx, const nyxhip_batch3d& b, size_t per_roi, uint64_t& chunk)
{
    size_t budget = 0;
    if (per_roi)
        if (int rc = vol_budget(ctx, b, ctx->d_vol.bytes, budget)) return rc;
    chunk = vol_chunk(per_roi, budget, b.n_roi);
    if (chunk == 0)
        return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, std::string(tx.label) + ": the workspace of one ROI (" + std::to_string(per_roi) + " bytes) does not fit max_device_bytes");
    if (per_roi) HIP_TRY(ctx, ctx->d_vol.reserve((size_t)chunk * per_roi, ctx->stream()));
    return NYXHIP_OK;
}

int vol_bin_launch(nyxhip_ctx* ctx, const VolArgs& v)
{
    hipStream_t st = ctx->stream();
    HIP_TRY(ctx, hipMemsetAsync(v.boxes, vol_background_level(v.grey_info), (size_t)v.n_roi * v.box_stride, st));
    return launched(ctx, launch_vol_bin(v, st), "volume binning kernel");
}

int vol_bin(nyxhip_ctx* ctx, const nyxhip_batch3d& b, uint64_t roi0, uint64_t n_roi, unsigned char* boxes, uint64_t box_stride, int grey_info, uint32_t max_px,
            uint32_t max_cells)
{
    VolArgs v;
    memset(&v, 0, sizeof(v));
    v.roi0 = roi0; v.n_roi = n_roi; v.px_offset = b.px_offset; v.x = b.x; v.y = b.y; v.z = b.z; v.inten = b.inten;
    v.bbox_w = b.bbox_w; v.bbox_h = b.bbox_h; v.bbox_d = b.bbox_d; v.vmin = b.min_inten; v.vmax = b.max_inten;
    v.grey_info = grey_info; v.status = ctx->d_status.as<int>(); v.boxes = boxes; v.box_stride = box_stride;
    v.max_cells = max_cells ? max_cells : 1u; v.max_px = max_px ? max_px : 1u;
    return vol_bin_launch(ctx, v);
}

// checks of the per-ROI arrays on the host (a host batch, or the copies of a device batch); the extrema they imply
int vol_scan(nyxhip_ctx* ctx, uint64_t nr, const uint64_t* off, const uint32_t* w, const uint32_t* h, const uint32_t* d, uint32_t& max_px, uint32_t& max_cells)
{
    max_px = 0; max_cells = 0;
    for (uint64_t r = 0; r < nr; r++) {
        if (off[r + 1] < off[r]) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "px_offset is not monotone");
        const uint64_t n = off[r + 1] - off[r];
        if (n > 0xFFFFFFFFull) return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "volumes: an ROI exceeds 2^32 - 1 voxels");
        if (w[r] > kVolMaxSide || h[r] > kVolMaxSide || d[r] > kVolMaxSide)
            return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "volumes: a box side exceeds " + std::to_string(kVolMaxSide));
        const uint64_t cells = (uint64_t)w[r] * h[r] * d[r];
        if (n && cells > kVolMaxCells)
            return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "volumes: a box exceeds " + std::to_string(kVolMaxCells) + " cells (256^3)");
        max_px = (uint32_t)std::max<uint64_t>(max_px, n);
        if (n) max_cells = (uint32_t)std::max<uint64_t>(max_cells, cells);
    }
    return NYXHIP_OK;
}

// what every volume entry does behind its own checks: the extrema (stated or derived), the box sides of the batch where the entry sizes
// its workspace by them (from the host arrays this function holds anyway; copied only for a device batch with stated extrema), the
// staging of a host batch into one device slab, `body` on the device batch, the copy back, the device status in the entry's words.
// `boxes`: the entry reads coordinates and boxes.
int vol_run(nyxhip_ctx* ctx, const VolTexts& tx, const nyxhip_batch3d* b, bool boxes, size_t ncol, double* out, size_t ld, const VolBody& body)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->n_roi == 0) return NYXHIP_OK;
    hipStream_t st = ctx->stream();
    const uint64_t nr = b->n_roi;
    // a batch without boxes (the intensity block alone): every ROI's box counts as one cell
    std::vector<uint32_t> ones;
    uint32_t max_px = b->max_px, max_cells = b->max_bbox_cells;
    VolSides sides = {{1u, 1u, 1u}, vdz_pitch(1u, 1u)};

    if (b->memory == NYXHIP_MEM_DEVICE) {
        const bool derive = max_px == 0;
        if (!derive && boxes && (max_cells == 0 || max_cells > kVolMaxCells))
            return max_cells ? fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "volumes: a box exceeds " + std::to_string(kVolMaxCells) + " cells (256^3)")
                             : fail(ctx, NYXHIP_ERR_INVALID_ARG, "max_px is stated and max_bbox_cells is not");
        if (derive || tx.sides) {                          // one copy of the boxes, and to derive of the offsets
            std::vector<uint64_t> off(derive ? nr + 1 : 0);
            std::vector<uint32_t> whd(3 * nr, 1u);
            if (derive) HIP_TRY(ctx, hipMemcpyAsync(off.data(), b->px_offset, 8 * (nr + 1), hipMemcpyDeviceToHost, st));
            if (boxes) {
                HIP_TRY(ctx, hipMemcpyAsync(whd.data(), b->bbox_w, 4 * nr, hipMemcpyDeviceToHost, st));
                HIP_TRY(ctx, hipMemcpyAsync(whd.data() + nr, b->bbox_h, 4 * nr, hipMemcpyDeviceToHost, st));
                HIP_TRY(ctx, hipMemcpyAsync(whd.data() + 2 * nr, b->bbox_d, 4 * nr, hipMemcpyDeviceToHost, st));
            }
            HIP_TRY(ctx, hipStreamSynchronize(st));
            if (derive)
                if (int rc = vol_scan(ctx, nr, off.data(), whd.data(), whd.data() + nr, whd.data() + 2 * nr, max_px, max_cells)) return rc;
            if (tx.sides) sides = vol_sides(nr, whd.data(), whd.data() + nr, whd.data() + 2 * nr, max_cells ? max_cells : 1u);
        }
        nyxhip_batch3d d = *b;
        if (!boxes) { d.x = d.y = d.z = nullptr; d.bbox_w = d.bbox_h = d.bbox_d = nullptr; }
        if (int rc = body(d, out, ld, max_px, max_cells, sides)) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return vol_check_status(ctx, tx);
    }

    // host batch: check the arrays, stage them into one device slab, run, copy the table back
    {
        const uint32_t* w = b->bbox_w; const uint32_t* h = b->bbox_h; const uint32_t* dd = b->bbox_d;
        if (!boxes) { ones.assign(nr, 1u); w = h = dd = ones.data(); }
        uint32_t dpx = 0, dcells = 0;
        if (int rc = vol_scan(ctx, nr, b->px_offset, w, h, dd, dpx, dcells)) return rc;
        if (max_px == 0) { max_px = dpx; max_cells = dcells; }
        else if (boxes && (max_cells == 0 || max_cells > kVolMaxCells)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "max_px is stated and max_bbox_cells is not (or exceeds 256^3)");
        if (tx.sides) sides = vol_sides(nr, w, h, dd, max_cells ? max_cells : 1u);
    }
    const uint64_t npx = b->px_offset[nr];
    const bool slide = b->slide_min != nullptr;
    const size_t o_off = 0, o_x = al256(o_off + 8 * (nr + 1)), o_y = al256(o_x + 2 * npx), o_z = al256(o_y + 2 * npx), o_i = al256(o_z + 2 * npx),
                 o_w = al256(o_i + 4 * npx), o_h = al256(o_w + 4 * nr), o_d = al256(o_h + 4 * nr), o_mn = al256(o_d + 4 * nr), o_mx = al256(o_mn + 4 * nr),
                 o_s0 = al256(o_mx + 4 * nr), o_s1 = al256(o_s0 + 8 * nr), o_out = al256(o_s1 + 8 * nr), total = al256(o_out + 8ull * nr * ncol);
    if (int rc = ensure_stage(ctx, total)) return rc;
    char* const base = ctx->d_stage.as<char>();
    HIP_TRY(ctx, hipMemcpyAsync(base + o_off, b->px_offset, 8 * (nr + 1), hipMemcpyHostToDevice, st));
    if (npx) {
        if (boxes) {
            HIP_TRY(ctx, hipMemcpyAsync(base + o_x, b->x, 2 * npx, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(base + o_y, b->y, 2 * npx, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(base + o_z, b->z, 2 * npx, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(ctx, hipMemcpyAsync(base + o_i, b->inten, 4 * npx, hipMemcpyHostToDevice, st));
    }
    if (boxes) {
        HIP_TRY(ctx, hipMemcpyAsync(base + o_w, b->bbox_w, 4 * nr, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(base + o_h, b->bbox_h, 4 * nr, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(base + o_d, b->bbox_d, 4 * nr, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(ctx, hipMemcpyAsync(base + o_mn, b->min_inten, 4 * nr, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_mx, b->max_inten, 4 * nr, hipMemcpyHostToDevice, st));
    if (slide) {
        HIP_TRY(ctx, hipMemcpyAsync(base + o_s0, b->slide_min, 8 * nr, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(base + o_s1, b->slide_max, 8 * nr, hipMemcpyHostToDevice, st));
    }
    nyxhip_batch3d d;
    memset(&d, 0, sizeof(d));
    d.n_roi = nr; d.memory = NYXHIP_MEM_DEVICE; d.max_device_bytes = b->max_device_bytes;
    d.px_offset = (const uint64_t*)(base + o_off);
    if (boxes) { d.x = (const uint16_t*)(base + o_x); d.y = (const uint16_t*)(base + o_y); d.z = (const uint16_t*)(base + o_z); }
    d.inten = (const uint32_t*)(base + o_i);
    if (boxes) { d.bbox_w = (const uint32_t*)(base + o_w); d.bbox_h = (const uint32_t*)(base + o_h); d.bbox_d = (const uint32_t*)(base + o_d); }
    d.min_inten = (const uint32_t*)(base + o_mn); d.max_inten = (const uint32_t*)(base + o_mx);
    if (slide) { d.slide_min = (const double*)(base + o_s0); d.slide_max = (const double*)(base + o_s1); }
    double* const d_out = (double*)(base + o_out);
    if (int rc = body(d, d_out, ncol, max_px, max_cells, sides)) { (void)hipStreamSynchronize(st); return rc; }
    HIP_TRY(ctx, hipMemcpy2DAsync(out, ld * sizeof(double), d_out, ncol * sizeof(double), ncol * sizeof(double), nr, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return vol_check_status(ctx, tx);
}

} // namespace nyxhip

extern "C" {

int nyxhip_vol_n_columns(uint32_t vmask, const nyxhip_settings* s)
{
    (void)s;
    return vol_mask_ok(vmask) ? vol_cols(vmask) : -1;
}

int nyxhip_vol_column_name(uint32_t vmask, const nyxhip_settings* s, int col, char* buf, size_t buf_len)
{
    (void)s;
    if (!buf || buf_len == 0 || !vol_mask_ok(vmask) || col < 0 || col >= vol_cols(vmask)) return NYXHIP_ERR_INVALID_ARG;
    if (vmask & NYXHIP_VFAM_INTENSITY) {
        if (col < kVolIntensityCols) { snprintf(buf, buf_len, "3%s", kVolIntensityNames[col]); return NYXHIP_OK; }
        col -= kVolIntensityCols;
    }
    if (col < kVolGlcmAngled * kVolDirs) snprintf(buf, buf_len, "3GLCM_%s_%d", kVolGlcmNames[col / kVolDirs], col % kVolDirs);
    else snprintf(buf, buf_len, "3GLCM_%s_AVE", kVolGlcmAveNames[col - kVolGlcmAngled * kVolDirs]);
    return NYXHIP_OK;
}

int nyxhip_featurize_volumes(nyxhip_ctx* ctx, const nyxhip_batch3d* b, uint32_t vmask, const nyxhip_settings* s, double* out, size_t ld)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    const bool glcm = (vmask & NYXHIP_VFAM_GLCM) != 0, inten = (vmask & NYXHIP_VFAM_INTENSITY) != 0;
    const size_t ncol = (size_t)vol_cols(vmask);
    if (int rc = vol_entry_checks(ctx, kTexts, b, s != nullptr, out, vol_mask_ok(vmask) ? nullptr : "bad volume mask: NYXHIP_VFAM_INTENSITY | NYXHIP_VFAM_GLCM are the bits it has",
                                  glcm, true, ncol, ld))
        return rc;
    if (inten) {
        if (s->grey_depth == 0) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "grey_depth must be non-zero (histogram bin count)");
        if ((uint32_t)abs(s->grey_depth) > kVolMaxHistBins)
            return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "volumes: the intensity histogram takes at most " + std::to_string(kVolMaxHistBins) + " bins");
    }
    if (glcm) {
        if (s->glcm_offset < 1) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "glcm_offset must be >= 1");
        if (!s->ibsi && (uint32_t)abs(s->glcm_grey_depth) > kVolLevelCap)
            return fail(ctx, NYXHIP_ERR_UNSUPPORTED, kTexts.cap + "; |glcm_grey_depth| = " + std::to_string(abs(s->glcm_grey_depth)) + " exceeds that cap");
    }
    return vol_run(ctx, kTexts, b, glcm, ncol, out, ld,
                   [&](const nyxhip_batch3d& d, double* d_out, size_t d_ld, uint32_t max_px, uint32_t max_cells, const VolSides&) {
                       return vol_device(ctx, &d, vmask, s, d_out, d_ld, max_px, max_cells);
                   });
}

} // extern "C"
