// nyxhip_contour.hip -- the families that have no size classes (kTailFams): the pixel-cloud launchers (caliper, chords, ellipse and
// erosion) and the contour chain with its readers (moments, radial, outline, circle).  Each kernel carves its LDS for a cap; the ROIs
// beyond it go through a deferred list (deferred_list.h).
#include "nyxhip_ctx.h"
#include "radial_close.h"
#include "deferred_list.h"

using namespace nyxhip;

namespace {

// The caliper classes (roi_caliper.hip) on `st`: one workgroup per ROI over the pixel clouds, no contour.  Columns: between
// FRACT_DIM_PERIMETER and EULER_NUMBER.  The origins are those the entry point left in the context (NULL: (0, 0)).  ROIs whose
// boxes are wider than the LDS column table go through a classifier and a list launch over global tables, like the outline
// kernel's deferred ROIs.
int launch_caliper(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_side,
                   hipStream_t st)
{
    CalArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.n_roi = b->n_roi;
    ca.px_offset = b->px_offset; ca.x = b->x; ca.y = b->y; ca.bbox_w = b->bbox_w;
    ca.origin_x = ctx->origin_x_next; ca.origin_y = ctx->origin_y_next;
    ca.out = d_out; ca.ld = ld; ca.status = ctx->d_status.as<int>();
    ca.fams = mask & kCaliper;
    ca.col_feret = nyxhip_n_columns(mask & (NYXHIP_FAM_INTENSITY | kEllipseErosion | NYXHIP_FAM_FRACTAL), s);
    ca.col_martin = ca.col_feret + ((mask & NYXHIP_FAM_FERET) ? kFeretCols : 0);
    ca.col_nassenstein = ca.col_martin + ((mask & NYXHIP_FAM_MARTIN) ? kMartinCols : 0);
    ca.soft_nan = s->soft_nan;
    // the reference's expression (rotation.cpp:56-58) on the host's libm, as the reference evaluates it
    for (int k = 0; k < kCaliperAngles; k++) {
        const float theta = (float)(10 * k) * float(3.14159265358979323846) / 180.f;
        ca.sn[k] = std::sin((double)theta); ca.cs[k] = std::cos((double)theta);
    }
    const uint32_t side = std::max<uint32_t>(max_side, 1u);
    ca.cols_cap = std::min<uint32_t>(kCaliperColsLds, (side + 7u) & ~7u);
    ca.defer_wide = side > kCaliperColsLds ? 1u : 0u;
    if (launch_roi_caliper(ca, st, (uint32_t)b->n_roi) != 0)
        return fail(ctx, NYXHIP_ERR_HIP, "caliper kernel: launch failed");
    if (!ca.defer_wide) return NYXHIP_OK;
    DeferredList wide;
    if (int rc = deferred_build(ctx, "caliper", ctx->d_caliper.list, b->n_roi, CaliperWide{b->bbox_w, ca.cols_cap}, st, wide)) return rc;
    if (int rc = deferred_count(ctx, wide, st)) return rc;
    if (!wide.hdr[0]) return NYXHIP_OK;
    const uint32_t ws_cols = (std::min<uint32_t>(side, 65535u) + 31u) & ~31u;
    const uint64_t stride = (uint64_t)kCaliperBytesPerCol * ws_cols;
    CalArgs cw = ca;
    cw.defer_wide = 0; cw.ws_cols = ws_cols;
    return deferred_chunks(ctx, "caliper", wide, stride, (size_t)1 << 30, ctx->d_caliper.ws, st, [&](const uint32_t* list, uint32_t count) {
        cw.ws = ctx->d_caliper.ws.as<unsigned char>(); cw.roi_index = list;
        return launch_roi_caliper(cw, st, count) != 0 ? fail(ctx, NYXHIP_ERR_HIP, "caliper kernel: launch failed") : NYXHIP_OK;
    });
}

// ChordsFeature (roi_chords.hip) on `st`: one workgroup per ROI over the pixel clouds, no contour.  Columns: between the Nassenstein
// columns and EULER_NUMBER.  The origins are those the entry point left in the context (NULL: (0, 0)).  ROIs whose rotated bit plane
// may exceed the LDS plane, and ROIs with zero-intensity pixels (min_inten == 0), go through a classifier and a list launch over
// global planes.  Which ROIs those are is known on the device only: the classifier's three counters are read back on every call
// (one stream synchronisation, as the caliper and outline kernels have for their wide boxes).
int launch_chords(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_side,
                  hipStream_t st)
{
    ChordArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.n_roi = b->n_roi;
    ca.px_offset = b->px_offset; ca.x = b->x; ca.y = b->y; ca.inten = b->inten; ca.bbox_w = b->bbox_w; ca.bbox_h = b->bbox_h;
    ca.min_inten = b->min_inten;
    ca.origin_x = ctx->origin_x_next; ca.origin_y = ctx->origin_y_next;
    ca.out = d_out; ca.ld = ld; ca.status = ctx->d_status.as<int>();
    ca.col0 = nyxhip_n_columns(mask & (NYXHIP_FAM_INTENSITY | kEllipseErosion | NYXHIP_FAM_FRACTAL | kCaliper), s);
    // the reference's loop (chords.cpp:22-23) and its expressions (rotation.cpp:70-82: the angle is passed as float) on the host's libm
    {
        const double step = M_PI / double(kChordsAngles);
        int k = 0;
        for (double ang = 0; ang < M_PI && k < kChordsAngles; ang += step, k++) {
            const float theta = (float)ang;
            ca.ang[k] = ang; ca.sn[k] = std::sin((double)theta); ca.cs[k] = std::cos((double)theta);
        }
        if (k != kChordsAngles)
            return fail(ctx, NYXHIP_ERR_HIP, "chords: the angle loop did not give 20 angles");
    }
    const uint32_t side = std::min<uint32_t>(std::max<uint32_t>(max_side, 1u), 65535u);
    ca.lds_words = (uint32_t)std::min<uint64_t>(kChordsLdsWords, chords_plane_words(side, side));
    DeferredList listed;
    if (int rc = deferred_build(ctx, "chords", ctx->d_chords.list, b->n_roi, ChordsListed{b->bbox_w, b->bbox_h, b->min_inten, ca.lds_words}, st, listed))
        return rc;
    if (launch_roi_chords(ca, st, (uint32_t)b->n_roi) != 0)                  // (queued ahead of the read-back: the host blocks with it running)
        return fail(ctx, NYXHIP_ERR_HIP, "chords kernel: launch failed");
    if (int rc = deferred_count(ctx, listed, st)) return rc;
    if (!listed.hdr[0]) return NYXHIP_OK;
    ChordArgs cw = ca;
    cw.ws_words = ((uint64_t)listed.hdr[1] + 63) & ~63ull;
    cw.ws_cells = ((uint64_t)listed.hdr[2] * listed.hdr[2] + 63) & ~63ull;
    const uint64_t stride = 4ull * (cw.ws_words + cw.ws_cells);
    return deferred_chunks(ctx, "chords", listed, stride, (size_t)1 << 30, ctx->d_chords.ws, st, [&](const uint32_t* list, uint32_t count) {
        cw.ws = ctx->d_chords.ws.as<uint32_t>(); cw.roi_index = list;
        return launch_roi_chords(cw, st, count) != 0 ? fail(ctx, NYXHIP_ERR_HIP, "chords kernel: launch failed") : NYXHIP_OK;
    });
}

// EllipseFittingFeature and ErosionPixelsFeature (roi_erosion.hip) on `st`, over the pixel clouds: no contour, no origin.  Columns:
// directly behind the intensity block.  The ellipse sums take a wave per ROI, and a workgroup per ROI of more than kEllipseWavePx
// pixels when the batch can hold one.  The erosion takes a workgroup per ROI with its two bit planes in LDS; when the batch's extrema
// allow a box beyond kErosionLdsWords, those ROIs go through a classifier and a list launch over global planes (the pattern of
// launch_caliper: one read-back, and only then).
int launch_ellipse_erosion(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px,
                           uint32_t max_area, uint32_t max_side, hipStream_t st)
{
    EroArgs ea;
    memset(&ea, 0, sizeof(ea));
    ea.n_roi = b->n_roi;
    ea.px_offset = b->px_offset; ea.x = b->x; ea.y = b->y; ea.bbox_w = b->bbox_w; ea.bbox_h = b->bbox_h;
    ea.min_inten = b->min_inten; ea.max_inten = b->max_inten;
    ea.out = d_out; ea.ld = ld; ea.status = ctx->d_status.as<int>();
    ea.col_ellipse = nyxhip_n_columns(mask & NYXHIP_FAM_INTENSITY, s);
    ea.col_erosion = ea.col_ellipse + ((mask & NYXHIP_FAM_ELLIPSE) ? kEllipseCols : 0);
    if (mask & NYXHIP_FAM_ELLIPSE) {
        const uint32_t most = max_px ? max_px : max_area;                      // (a batch without a stated pixel maximum: no ROI has more than its box)
        if (launch_roi_ellipse(ea, st, most > kEllipseWavePx) != 0)
            return fail(ctx, NYXHIP_ERR_HIP, "ellipse kernel: launch failed");
    }
    if (!(mask & NYXHIP_FAM_EROSION)) return NYXHIP_OK;
    // bound of two planes over boxes of at most max_area cells and max_side a side: (w / 32 + 1) * h <= area / 32 + side
    const uint64_t bound = std::max<uint64_t>(2ull * ((uint64_t)max_area / 32u + max_side), 2u);
    ea.lds_words = (uint32_t)std::min<uint64_t>(kErosionLdsWords, bound);
    ea.defer_large = bound > kErosionLdsWords ? 1u : 0u;
    if (launch_roi_erosion(ea, st, (uint32_t)b->n_roi) != 0)
        return fail(ctx, NYXHIP_ERR_HIP, "erosion kernel: launch failed");
    if (!ea.defer_large) return NYXHIP_OK;
    DeferredList listed;
    if (int rc = deferred_build(ctx, "erosion", ctx->d_erosion.list, b->n_roi, ErosionListed{b->bbox_w, b->bbox_h, ea.lds_words}, st, listed)) return rc;
    if (int rc = deferred_count(ctx, listed, st)) return rc;
    if (!listed.hdr[0]) return NYXHIP_OK;
    EroArgs ew = ea;
    ew.defer_large = 0;
    ew.ws_stride = (2ull * listed.hdr[1] + 63) & ~63ull;
    return deferred_chunks(ctx, "erosion", listed, 4 * ew.ws_stride, (size_t)1 << 30, ctx->d_erosion.ws, st, [&](const uint32_t* list, uint32_t count) {
        ew.ws = ctx->d_erosion.ws.as<uint32_t>(); ew.roi_index = list;
        return launch_roi_erosion(ew, st, count) != 0 ? fail(ctx, NYXHIP_ERR_HIP, "erosion kernel: launch failed") : NYXHIP_OK;
    });
}

// Contour (roi_moments.hip) + the families that read it: the 2-D geometric moments (roi_moments.hip) and the radial intensity
// distribution (roi_radial.hip).  The contour of every ROI goes to a context-owned workspace at the ROI's CSR offset (a contour
// never has more points than the ROI has pixels) ONCE per call; the moments kernel and / or the radial kernel read it back.
// (The workspace keeps its per-pixel double plane for a radial-only call too: the contour kernel's walk stack lives there.)
// The outline kernel (roi_outline.hip) is the third reader, the circle kernel (roi_circle.hip) the fourth; a mask that holds none of the contour families (EULER_NUMBER alone) skips
// the contour chain and launches it by itself.  allow_lane = false: everything stays on the call's stream (the caller has joined the
// lanes: the feature kernels of a GLCM launch zero the outline columns, so the outline kernel must follow all of them).
// contour_out != NULL: the contour chain runs whatever the mask holds (0: the chain alone, no reader, d_out unused) and the argument
// block that names its workspace (ws_contour / n_contour) is handed back -- the neighbor entries read the contours themselves.
} // namespace

int nyxhip::launch_contour_families(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* d_out, size_t ld,
                                    uint32_t max_px, uint32_t max_area, uint32_t max_side, bool allow_lane, MomArgs* contour_out)
{
    hipStream_t st = ctx->stream();
    const bool do_out = (mask & kOutline) != 0, need_contour = (mask & kContourFams) != 0 || contour_out != nullptr;
    OutArgs oa;
    memset(&oa, 0, sizeof(oa));
    bool out_deferred = false;                             // some ROI's bit planes may exceed LDS: a list launch follows the readers
    if (do_out) {
        oa.fams = mask & kOutline;
        oa.has_contour = need_contour ? 1u : 0u;
        oa.col_fractal = nyxhip_n_columns(mask & (NYXHIP_FAM_INTENSITY | kEllipseErosion), s);   // (the ellipse and erosion columns precede it)
        oa.col_euler = oa.col_fractal + ((mask & NYXHIP_FAM_FRACTAL) ? kFractalCols : 0) + nyxhip_n_columns(mask & (kCaliper | NYXHIP_FAM_CHORDS), s);   // (enum order)
        oa.col_radius = oa.col_euler + ((mask & NYXHIP_FAM_EULER) ? kEulerCols : 0) + nyxhip_n_columns(mask & kCircleGeodetic, s);   // (the circle and geodetic columns precede it)
        if (mask & (NYXHIP_FAM_FRACTAL | NYXHIP_FAM_EULER)) {
            // bound of outline_bit_words over boxes of at most max_area cells and max_side a side: rows of w / 32 + 1 words, the pyramid
            // at most as much again plus a word and a row per level
            const uint64_t bound = 2ull * ((uint64_t)max_area / 32u + max_side) + 2ull * max_side + 64u;
            oa.bits_cap = (uint32_t)std::min<uint64_t>(kOutlineBitsLds, bound);
            out_deferred = bound > kOutlineBitsLds;
            oa.defer_bits = out_deferred ? 1u : 0u;
        }
    }
    // the ROIs the outline launches deferred, from global bit planes: on `s_`, behind everything that wrote their contours
    auto launch_outline_deferred = [&](hipStream_t s_) -> int {
        if (!out_deferred) return NYXHIP_OK;
        const uint32_t pyramid = (mask & NYXHIP_FAM_FRACTAL) ? 1u : 0u;
        DeferredList big;
        if (int rc = deferred_build(ctx, "outline", ctx->d_outline.list, b->n_roi, OutlineBitsBig{b->bbox_w, b->bbox_h, pyramid, oa.bits_cap}, s_, big))
            return rc;
        if (int rc = deferred_count(ctx, big, s_)) return rc;
        if (!big.hdr[0]) return NYXHIP_OK;
        const uint32_t sd = std::min<uint32_t>(max_side, 65535u);
        const uint64_t stride = (std::min<uint64_t>(2ull * ((uint64_t)max_area / 32u + max_side) + 2ull * max_side + 64u, outline_bit_words(sd, sd, pyramid != 0)) + 63) & ~63ull;
        OutArgs ob = oa;
        ob.defer_bits = 0; ob.bits_stride = stride;
        ob.m.sp.defer_large = 0;
        return deferred_chunks(ctx, "outline", big, 4 * stride, (size_t)1 << 30, ctx->d_outline.ws, s_, [&](const uint32_t* list, uint32_t count) {
            ob.bits_ws = ctx->d_outline.ws.as<uint32_t>(); ob.m.sp.roi_index = list;
            return launch_roi_outline(ob, s_, count) != 0 ? fail(ctx, NYXHIP_ERR_HIP, "outline kernel: launch failed") : NYXHIP_OK;
        });
    };
    // the circle / geodetic classes (roi_circle.hip): the fourth reader of the contour, columns directly behind EULER_NUMBER
    const bool do_circ = (mask & kCircleGeodetic) != 0;
    CircArgs cg;
    memset(&cg, 0, sizeof(cg));
    if (do_circ) {
        cg.fams = mask & kCircleGeodetic;
        cg.col_circles = nyxhip_n_columns(mask & (NYXHIP_FAM_INTENSITY | kEllipseErosion | NYXHIP_FAM_FRACTAL | kCaliper | NYXHIP_FAM_CHORDS | NYXHIP_FAM_EULER), s);
        cg.col_geodetic = cg.col_circles + ((mask & NYXHIP_FAM_CIRCLES) ? kCirclesCols : 0);
        cg.origin_x = ctx->origin_x_next; cg.origin_y = ctx->origin_y_next;
    }
    if (mask & kCaliper)
        if (int crc = launch_caliper(ctx, b, mask, s, d_out, ld, max_side, st)) return crc;
    if (mask & NYXHIP_FAM_CHORDS)
        if (int crc = launch_chords(ctx, b, mask, s, d_out, ld, max_side, st)) return crc;
    if (mask & kEllipseErosion)
        if (int crc = launch_ellipse_erosion(ctx, b, mask, s, d_out, ld, max_px, max_area, max_side, st)) return crc;
    if (!need_contour && !do_out)
        return NYXHIP_OK;                                  // the caliper classes / the chords / the ellipse and erosion classes alone
    if (!need_contour) {
        // EULER_NUMBER alone: no contour, no staged pixels -- the bit plane only
        MomArgs& m = oa.m;
        m.n_roi = b->n_roi;
        m.px_offset = b->px_offset; m.x = b->x; m.y = b->y; m.inten = b->inten; m.bbox_w = b->bbox_w; m.bbox_h = b->bbox_h;
        m.out = d_out; m.ld = ld; m.status = ctx->d_status.as<int>();
        if (launch_roi_outline(oa, st, (uint32_t)b->n_roi) != 0)
            return fail(ctx, NYXHIP_ERR_HIP, "outline kernel: launch failed");
        return launch_outline_deferred(st);
    }
    // A batch with boxes beyond the LDS plane sends those to a wave per ROI over a global workspace (a few hundred waves, ~10 ms of
    // latency for the heavy-tailed batch): with other families in the call the whole moments chain goes to a lane of its own and
    // runs beside them (enqueued last, dependent only on the batch).  Its scratch is the lane's, not the main stream's.
    const bool big_boxes = (uint64_t)kContourWaves * (((uint64_t)max_area + 4ull * max_side + 4 + 15) & ~15ull) > (uint64_t)roi_features_max_lds();
    const bool on_lane = allow_lane && !knob::no_mom_lane() && big_boxes && (mask & ~kTailFams) && ctx->lane_fork;
    if (on_lane)
        if (int lrc = use_lane(ctx, nyxhip_ctx::kMomLane, &st)) return lrc;
    DevBuf& spill = on_lane ? ctx->lane_buf[nyxhip_ctx::kMomLane] : ctx->d_spill;
    uint64_t total_px = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total_px, b->px_offset + b->n_roi, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_k = 0, o_n = al(4 * (size_t)total_px + 256), o_l = al(o_n + 4 * (size_t)b->n_roi + 256), need = al(o_l + 8 * (size_t)total_px + 256);
    HIP_TRY(ctx, ctx->d_mom.reserve(need, st, need + need / 8));
    char* base = ctx->d_mom.as<char>();
    MomArgs m;
    memset(&m, 0, sizeof(m));
    m.n_roi = b->n_roi;
    m.px_offset = b->px_offset; m.x = b->x; m.y = b->y; m.inten = b->inten; m.bbox_w = b->bbox_w; m.bbox_h = b->bbox_h;
    m.out = d_out; m.ld = ld; m.status = ctx->d_status.as<int>();
    m.mask = mask & kMoments;
    m.col_smoms = nyxhip_n_columns(mask & ~kMoments, s);     // (every other family, the radial distribution included, precedes the moments)
    m.col_imoms = m.col_smoms + ((mask & NYXHIP_FAM_SMOMS) ? kMomCols : 0);
    m.ws_contour = (uint32_t*)(base + o_k); m.n_contour = (uint32_t*)(base + o_n); m.ws_L = (double*)(base + o_l);
    if (!ctx->d_logtab) {                                 // log(sqrt(d) + 0.001), d < 32768: boxes up to 128 x 128 never evaluate a logarithm
        constexpr uint32_t kLogTab = 32768;
        HIP_TRY(ctx, ctx->d_logtab.reserve(8ull * kLogTab, nullptr));
        if (launch_moments_logtab(ctx->d_logtab.as<double>(), kLogTab, st) != 0) return fail(ctx, NYXHIP_ERR_HIP, "moments log table: launch failed");
        ctx->logtab_n = kLogTab;
    }
    m.log_tab = ctx->d_logtab.as<double>(); m.log_tab_n = ctx->logtab_n;
    // LDS of the moments kernel from the batch extrema: every pixel of the largest ROI (up to kMomPxLds; larger ROIs sweep HBM),
    // a contour of up to the bounding box's perimeter (what a convex ROI can have; longer ones are read from HBM), its step table
    m.px_cap = std::min<uint32_t>((uint32_t)kMomPxLds, (std::max<uint32_t>(max_px ? max_px : max_area, 1u) + 7u) & ~7u);
    m.k_cap = std::min<uint32_t>((uint32_t)kMomContourLds, std::max<uint32_t>(256u, (4u * std::min<uint32_t>(max_side, 65536u) + 63u) & ~63u));
    m.step_cap = std::min<uint32_t>((uint32_t)kMomStepTab, m.k_cap);
    const bool do_mom = (mask & kMoments) != 0, do_rad = (mask & NYXHIP_FAM_RADIAL) != 0;
    RadArgs ra;
    memset(&ra, 0, sizeof(ra));
    if (do_rad) {
        // columns: FRAC_AT_D | GABOR | MEAN_FRAC | RADIAL_CV (enum order)
        const uint32_t before = NYXHIP_FAM_INTENSITY | kBehindIntensity | NYXHIP_FAM_GLCM | kTexture | kDependence;
        ra.col_frac = nyxhip_n_columns(mask & before, s);
        ra.col_mean = ra.col_frac + kRadialBins + ((mask & NYXHIP_FAM_GABOR) ? s->gabor_n_filters : 0);
        ra.col_cv = ra.col_mean + kRadialBins;
        ra.wedge_tab = radial_wedge_tab();                 // the eight boundary directions on the host's libm (radial_close.h)
    }
    // the readers of a contour launch, on its stream: the moments of `mm` and / or the radial distribution over the same ROIs
    auto launch_readers = [&](const MomArgs& mm, hipStream_t s_, uint32_t g) -> int {
        int r = do_mom ? launch_roi_moments(mm, s_, g) : 0;
        if (r == 0 && do_rad) {
            ra.m = mm;
            r = launch_roi_radial(ra, s_, g);
        }
        if (r == 0 && do_out) {
            oa.m = mm;
            r = launch_roi_outline(oa, s_, g);
        }
        if (r == 0 && do_circ) {
            cg.m = mm;
            r = launch_roi_circle(cg, s_, g);
        }
        return r;
    };
    const uint64_t full_plane = (uint64_t)max_area + 4ull * max_side + 4;      // (w + 2)(h + 2) <= area + 2(w + h) + 4
    const uint32_t grid = (uint32_t)b->n_roi;
    const uint32_t lds_cap = (uint32_t)roi_features_max_lds();
    int rc;
    auto launch_failed = [&](int hrc) {
        return fail(ctx, NYXHIP_ERR_HIP, std::string("contour / moments / radial / outline / circle kernel launch failed: ") + hipGetErrorString((hipError_t)hrc));
    };
    hipStream_t st_join = nullptr;                         // the big boxes' stream when it is not `st`
    if ((uint64_t)kContourWaves * ((full_plane + 15) & ~15ull) <= lds_cap) {   // kContourWaves planes per workgroup
        m.plane_cap = (uint32_t)full_plane;
        rc = launch_roi_contour(m, st, grid);
        if (rc == 0) rc = launch_readers(m, st, grid);
    } else {
        // the bulk of the batch from LDS (16 KiB planes keep ten waves per CU), the oversized ROIs from a global workspace: a wave per ROI,
        // a few hundred waves and ~10 ms of latency for the heavy-tailed batch.  Two independent chains -- big boxes: list, contour over the
        // workspace, moments of the list | bulk: contour from LDS (skipping the big boxes), moments of everybody else -- on two lanes when
        // the call has lanes (other families to run beside), one after the other on the call's stream otherwise.
        m.plane_cap = 16 * 1024;
        hipStream_t st_big = st;
        if (on_lane)
            if (int lrc = use_lane(ctx, nyxhip_ctx::kMomLaneBig, &st_big)) return lrc;
        if (st_big != st) st_join = st_big;
        DeferredList large;
        if (int brc = deferred_build(ctx, "contour", ctx->d_spill_list, b->n_roi, ContourPlaneBig{b->bbox_w, b->bbox_h, m.plane_cap}, st_big, large))
            return brc;
        if (int brc = deferred_count(ctx, large, st_big)) return brc;
        rc = 0;
        if (large.hdr[0]) {
            if (full_plane > 0xFFFFFFF0ull) return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "bounding box too large for the contour plane");
            const size_t stride = al((size_t)full_plane);
            MomArgs m2 = m;
            m2.plane_cap = (uint32_t)full_plane;
            m2.sp.defer_large = 0;
            m2.sp.stride = stride;
            if (int crc = deferred_chunks(ctx, "contour", large, stride, (size_t)4 << 30, spill, st_big, [&](const uint32_t* list, uint32_t count) {
                    m2.sp.scratch = spill.as<unsigned char>(); m2.sp.roi_index = list;
                    const int hrc = launch_roi_contour(m2, st_big, count);
                    return hrc != 0 ? launch_failed(hrc) : NYXHIP_OK;
                }))
                return crc;
            MomArgs m3 = m;                                   // moments of the big boxes: the list
            m3.sp.roi_index = large.list();
            rc = launch_readers(m3, st_big, large.hdr[0]);
        }
        if (rc == 0) {
            m.sp.defer_large = 1;                             // both kernels skip the big boxes
            rc = launch_roi_contour(m, st, grid);
            if (rc == 0) rc = launch_readers(m, st, grid);
        }
    }
    if (rc != 0)
        return launch_failed(rc);
    if (contour_out) *contour_out = m;
    if (out_deferred) {
        if (st_join) {                                     // the deferred ROIs' contours may come from the big boxes' lane
            HIP_TRY(ctx, hipEventRecord(ctx->lane_done[nyxhip_ctx::kMomLaneBig], st_join));
            HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->lane_done[nyxhip_ctx::kMomLaneBig], 0));
        }
        oa.m = m;
        return launch_outline_deferred(st);
    }
    return NYXHIP_OK;
}
