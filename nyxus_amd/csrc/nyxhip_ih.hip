// nyxhip_ih.hip -- the intensity-histogram entries of include/nyxhip.h: column names, the launches over a device-resident batch (ih_device) and
// nyxhip_ih_batch.  The tile entry (nyxhip_ih_tiles) lives with the tile path in nyxhip_tiles.hip.
#include "nyxhip_ctx.h"
#include "batch_stage.h"

using namespace nyxhip;

namespace nyxhip {

static const char* const kIhNames[kIhCols] = {
    "IH_MEAN_VAL", "IH_VARIANCE_VAL", "IH_SKEWNESS_VAL", "IH_EXCESS_KURTOSIS_VAL", "IH_MEDIAN_VAL", "IH_MINIMUM_VAL", "IH_P10_VAL", "IH_P90_VAL",
    "IH_MAXIMUM_VAL", "IH_MODE_VAL", "IH_INTERQUANTILE_RANGE_VAL", "IH_RANGE_VAL", "IH_MEAN_ABSOLUTE_DEVIATION_VAL",
    "IH_ROBUST_MEAN_ABSOLUTE_DEVIATION_VAL", "IH_MEDIAN_ABSOLUTE_DEVIATION_VAL", "IH_COEFFICIENT_OF_VARIATION_VAL",
    "IH_QUANTILE_COEFFICIENT_OF_DISPERSION_VAL", "IH_ENTROPY_VAL", "IH_UNIFORMITY_VAL", "IH_ROBUST_MEAN_VAL",
    "IH_MEAN_IDX", "IH_VARIANCE_IDX", "IH_SKEWNESS_IDX", "IH_EXCESS_KURTOSIS_IDX", "IH_MEDIAN_IDX", "IH_MINIMUM_IDX", "IH_P10_IDX", "IH_P90_IDX",
    "IH_MAXIMUM_IDX", "IH_MODE_IDX", "IH_INTERQUANTILE_RANGE_IDX", "IH_RANGE_IDX", "IH_MEAN_ABSOLUTE_DEVIATION_IDX",
    "IH_ROBUST_MEAN_ABSOLUTE_DEVIATION_IDX", "IH_MEDIAN_ABSOLUTE_DEVIATION_IDX", "IH_COEFFICIENT_OF_VARIATION_IDX",
    "IH_QUANTILE_COEFFICIENT_OF_DISPERSION_IDX", "IH_ENTROPY_IDX", "IH_UNIFORMITY_IDX",
    "IH_MAX_GRADIENT", "IH_MAX_GRADIENT_IDX", "IH_MIN_GRADIENT", "IH_MIN_GRADIENT_IDX", "IH_ROBUST_MEAN_IDX", "IH_NUM_BINS", "IH_BIN_SIZE"};

int ih_settings_check(nyxhip_ctx* ctx, const nyxhip_settings* s)
{
    if (s->ibsi && s->grey_depth > kIhMaxBins)
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "intensity histogram: grey_depth beyond 4096 bins (the counters of a workgroup's ROIs live in 64 KiB of LDS)");
    return NYXHIP_OK;
}

int ih_device(nyxhip_ctx* ctx, const nyxhip_batch* b, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px)
{
    if (b->n_roi == 0) return NYXHIP_OK;
    if (int rc = ih_settings_check(ctx, s)) return rc;
    // A/B knob of tools/ih_probe.py: every ROI through the workgroup form
    const bool one_form = knob::ih_one_form();
    IhArgs a;
    memset(&a, 0, sizeof(a));
    a.n_roi = b->n_roi; a.px_offset = b->px_offset; a.inten = b->inten; a.vmin = b->min_inten; a.vmax = b->max_inten;
    a.n_bins = s->grey_depth; a.ibsi = s->ibsi; a.soft_nan = s->soft_nan; a.out = d_out; a.ld = ld;
    a.wave_px = one_form ? 0u : kIhWavePx;
    // max_px == 0: not known.  Every ROI belongs to exactly one form; a form without a member is not launched when that is known.
    // (An empty ROI belongs to the wave form, which writes its soft_nan row.)
    const bool block_form = max_px == 0 || max_px > a.wave_px;
    if (int rc = launch_roi_ih(a, ctx->stream(), true, block_form))
        return fail(ctx, NYXHIP_ERR_HIP, std::string("intensity-histogram kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
    return NYXHIP_OK;
}

} // namespace nyxhip

extern "C" {

int nyxhip_ih_column_name(int col, char* buf, size_t buf_len)
{
    if (!buf || buf_len == 0 || col < 0 || col >= kIhCols) return NYXHIP_ERR_INVALID_ARG;
    snprintf(buf, buf_len, "%s", kIhNames[col]);
    return NYXHIP_OK;
}

int nyxhip_ih_batch(nyxhip_ctx* ctx, const nyxhip_batch* b, const nyxhip_settings* s, double* out, size_t ld)
{
    const BatchSpec sp{kReadInten | kReadRange,
                       "batch has null array pointers (the intensity-histogram entries read px_offset, inten, min_inten, max_inten)", kIhCols};
    if (int rc = batch_check(ctx, sp, b, s, out, ld)) return rc;
    if (int rc = ih_settings_check(ctx, s)) return rc;
    return batch_run(ctx, sp, b, out, ld, [&](const StagedBatch& g) {
        // the largest ROI: a host batch's at least 1 (known), a device batch's as stated (0: not known)
        return ih_device(ctx, &g.d, s, g.d_out, g.ld, g.host ? std::max(g.max_px, 1u) : g.max_px);
    });
}

} // extern "C"
