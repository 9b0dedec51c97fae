// batch_stage.h -- the host plumbing every batch entry shares (internal, host units): the argument checks, and a batch brought in front of
// the entry's device function -- a device batch as it is, a host batch walked, staged into one slab of nyxhip_ctx::d_stage and its table
// copied back.  An entry is: batch_check, the checks of its class alone, batch_run around a call of its *_device function.
#pragma once
#include "nyxhip_ctx.h"

namespace nyxhip __attribute__((visibility("hidden"))) {

// the arrays of nyxhip_batch a class reads besides px_offset
enum : uint32_t {
    kReadLabel = 1u << 0,              // roi_label
    kReadXY = 1u << 1,                 // x, y
    kReadInten = 1u << 2,              // inten
    kReadBox = 1u << 3,                // bbox_w, bbox_h
    kReadRange = 1u << 4,              // min_inten, max_inten
    kReadSlide = 1u << 5,              // slide_min, slide_max, where the batch gives them
};

struct BatchSpec {                     // what an entry states
    uint32_t reads;
    const char* null_arrays;           // the entry's words for a missing array
    int n_cols;
    const uint32_t *origin_x = nullptr, *origin_y = nullptr;                  // optional, in the batch's memory
    const uint64_t* image_offset = nullptr;                                   // optional CSR over the rows, in the batch's memory
    uint64_t n_images = 0;
    int (*status)(nyxhip_ctx*) = check_status;                                // the status check behind the run
};
struct NoRoiCheck { int operator()(uint64_t) const { return NYXHIP_OK; } };

struct StagedBatch {                   // what the entry's device call gets
    nyxhip_batch d;                    // device-resident
    const uint32_t *d_ox, *d_oy;
    const uint64_t* d_image_offset;
    double* d_out;
    size_t ld;
    bool host;                         // staged from a host batch: the extrema below are those of the walk (0 where no ROI has a pixel or a box)
    bool hinted;                       // ... or a device batch's statement, complete (max_px, max_area, max_side all non-zero) or not
    uint32_t max_px, max_area, max_side, max_range;
    uint64_t n_small;                  // host batch: ROIs of the smallest size class
};

inline int batch_check(nyxhip_ctx* ctx, const BatchSpec& sp, const nyxhip_batch* b, const nyxhip_settings* s, const double* out, size_t ld)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (!b || !s || !out) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null batch / settings / out_table");
    if ((sp.origin_x == nullptr) != (sp.origin_y == nullptr))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "origin_x and origin_y must both be given or both NULL");
    const uint32_t r = sp.reads;
    if (b->n_roi && (!b->px_offset || ((r & kReadLabel) && !b->roi_label) || ((r & kReadXY) && (!b->x || !b->y)) || ((r & kReadInten) && !b->inten) ||
                     ((r & kReadBox) && (!b->bbox_w || !b->bbox_h)) || ((r & kReadRange) && (!b->min_inten || !b->max_inten))))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, sp.null_arrays);
    if (ld < (size_t)sp.n_cols) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    if (b->n_roi > 0x7FFFFFFFull) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "too many ROIs in one batch");
    if (sp.image_offset && sp.n_images == 0) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "image_offset given with n_images == 0");
    if (b->memory != NYXHIP_MEM_DEVICE && b->memory != NYXHIP_MEM_HOST) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad batch->memory");
    return NYXHIP_OK;
}

// run(const StagedBatch&) enqueues the class's launches on the context's stream; the table is in `out` when this returns.
// roi_check(r): a check one class alone makes on ROI r of a host batch (a code of its own fail() call, or NYXHIP_OK).
template <class Run, class RoiCheck = NoRoiCheck>
int batch_run(nyxhip_ctx* ctx, const BatchSpec& sp, const nyxhip_batch* b, double* out, size_t ld, Run&& run, RoiCheck roi_check = RoiCheck())
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->n_roi == 0) return NYXHIP_OK;
    hipStream_t st = ctx->stream();
    StagedBatch g;
    memset(&g, 0, sizeof(g));
    if (b->memory == NYXHIP_MEM_DEVICE) {
        g.d = *b; g.d_ox = sp.origin_x; g.d_oy = sp.origin_y; g.d_image_offset = sp.image_offset; g.d_out = out; g.ld = ld;
        g.max_px = b->max_px; g.max_area = b->max_bbox_area; g.max_side = b->max_bbox_side; g.max_range = b->max_inten_range;
        g.hinted = b->max_px != 0 && b->max_bbox_area != 0 && b->max_bbox_side != 0;
        if (int rc = run(g)) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return sp.status(ctx);
    }
    // ---- the walk: px_offset is a CSR array of ROIs below 2^32 pixels; the batch extrema and the census of the smallest size class
    const uint64_t nr = b->n_roi, npx = b->px_offset[nr];
    g.host = g.hinted = true;
    const bool xy = sp.reads & kReadXY, box = sp.reads & kReadBox, range = sp.reads & kReadRange, slide = (sp.reads & kReadSlide) && b->slide_min;
    for (uint64_t r = 0; r < nr; r++) {
        if (b->px_offset[r + 1] < b->px_offset[r]) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "px_offset is not monotone");
        const uint64_t n = b->px_offset[r + 1] - b->px_offset[r];
        if (n > 0xFFFFFFFFull) return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "ROI exceeds 2^32 pixels");
        if (int rc = roi_check(r)) return rc;
        g.max_px = std::max(g.max_px, (uint32_t)n);
        if (!box) continue;
        const uint32_t w = b->bbox_w[r], h = b->bbox_h[r];
        if ((uint64_t)w * h > 0xFFFFFFFFull) return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "ROI exceeds 2^32 pixels");
        g.max_area = std::max(g.max_area, w * h);
        g.max_side = std::max(g.max_side, std::max(w, h));
        if (n <= kClassPx[0] && w <= kClassSide[0] && h <= kClassSide[0]) g.n_small++;
    }
    for (uint64_t r = 0; range && r < nr; r++) g.max_range = std::max(g.max_range, b->max_inten[r] - b->min_inten[r]);
    if (sp.image_offset) {
        if (sp.image_offset[0] != 0 || sp.image_offset[sp.n_images] != nr) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "image_offset must run from 0 to n_roi");
        for (uint64_t k = 0; k < sp.n_images; k++)
            if (sp.image_offset[k + 1] < sp.image_offset[k]) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "image_offset is not monotone");
    }
    // ---- the slab: every array the class reads at a 256-byte boundary, the table behind them
    struct Part { const void* src; size_t bytes, at; };
    size_t o = 0;
    auto part = [&](bool read, const void* src, size_t bytes) {
        const Part p{read ? src : nullptr, read ? bytes : 0, o};
        o = (o + p.bytes + 255) & ~(size_t)255;
        return p;
    };
    enum { kOff, kX, kY, kInten, kBw, kBh, kLabel, kMin, kMax, kSmin, kSmax, kOx, kOy, kImg, kParts };
    const Part P[kParts] = {part(true, b->px_offset, 8 * (nr + 1)), part(xy, b->x, 2 * npx), part(xy, b->y, 2 * npx),
                            part(sp.reads & kReadInten, b->inten, 4 * npx), part(box, b->bbox_w, 4 * nr), part(box, b->bbox_h, 4 * nr),
                            part(sp.reads & kReadLabel, b->roi_label, 4 * nr), part(range, b->min_inten, 4 * nr), part(range, b->max_inten, 4 * nr),
                            part(slide, b->slide_min, 8 * nr), part(slide, b->slide_max, 8 * nr), part(sp.origin_x, sp.origin_x, 4 * nr),
                            part(sp.origin_x, sp.origin_y, 4 * nr), part(sp.image_offset, sp.image_offset, 8 * (sp.n_images + 1))};
    const size_t o_out = o;
    if (int rc = ensure_stage(ctx, o_out + (((size_t)8 * nr * sp.n_cols + 255) & ~(size_t)255))) return rc;
    char* const base = ctx->d_stage.as<char>();
    for (const Part& p : P)
        if (p.bytes) HIP_TRY(ctx, hipMemcpyAsync(base + p.at, p.src, p.bytes, hipMemcpyHostToDevice, st));
    auto dev = [&](int k) -> const void* { return P[k].src ? base + P[k].at : nullptr; };
    g.d.n_roi = nr; g.d.memory = NYXHIP_MEM_DEVICE;
    g.d.px_offset = (const uint64_t*)dev(kOff); g.d.x = (const uint16_t*)dev(kX); g.d.y = (const uint16_t*)dev(kY); g.d.inten = (const uint32_t*)dev(kInten);
    g.d.bbox_w = (const uint32_t*)dev(kBw); g.d.bbox_h = (const uint32_t*)dev(kBh); g.d.roi_label = (const uint32_t*)dev(kLabel);
    g.d.min_inten = (const uint32_t*)dev(kMin); g.d.max_inten = (const uint32_t*)dev(kMax);
    g.d.slide_min = (const double*)dev(kSmin); g.d.slide_max = (const double*)dev(kSmax);
    g.d_ox = (const uint32_t*)dev(kOx); g.d_oy = (const uint32_t*)dev(kOy); g.d_image_offset = (const uint64_t*)dev(kImg);
    g.d_out = (double*)(base + o_out); g.ld = (size_t)sp.n_cols;
    if (int rc = run(g)) return rc;
    // ---- the table, to the caller's leading dimension
    HIP_TRY(ctx, hipMemcpy2DAsync(out, ld * sizeof(double), g.d_out, g.ld * sizeof(double), g.ld * sizeof(double), nr, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return sp.status(ctx);
}

} // namespace nyxhip
