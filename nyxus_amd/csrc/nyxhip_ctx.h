// nyxhip_ctx.h -- what the host units of the library share (internal): the context behind include/nyxhip.h, the owner types of its
// device and pinned memory, error reporting, and the functions the units call in each other.
//   nyxhip_columns.hip   column catalogue, settings checks, defaults
//   nyxhip_dispatch.hip  layouts, argument blocks, size classes: a device-resident batch -> kernel launches
//   nyxhip_contour.hip   the families without size classes: pixel-cloud and contour launchers, their deferred lists (deferred_list.h)
//   nyxhip_tiles.hip     the fused tile path and its host staging
//   nyxhip_slides.hip    whole-slide mode: nyxhip_featurize_slides (one ROI per slide, no label image)
//   nyxhip_api.hip       context life cycle, the batch entry points, timing, launch report
//   batch_stage.h        what every batch entry shares: argument checks, a host batch staged into one slab, its table copied back
//   nyxhip_neighbors.hip the neighbor entries: column names, the launches over a device-resident batch, nyxhip_neighbors_batch
//   nyxhip_ih.hip        the intensity-histogram entries: column names, the launches over a device-resident batch, nyxhip_ih_batch
//   nyxhip_imq.hip       the image-quality entries: column names, the launches over a device-resident batch, nyxhip_imq_batch / _slides
//   nyxhip_morph.hip     the 2-D morphology entries: column catalogue of a morphology mask, the launches over a device-resident batch, nyxhip_morph_batch
//   nyxhip_hexpoly.hip   the hexagonality / polygonality entries: column names, one contour chain for three producers and the closing kernel, nyxhip_hexpoly_batch
//   nyxhip_vol.hip       the volume entries: column catalogue of the volume mask, chunks under the budget, nyxhip_featurize_volumes
//   nyxhip_volscan.hip   the device label scan for volumes: nyxhip_assemble_volumes, nyxhip_assembled_rows, nyxhip_release_volumes (vol_assembly.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <string>
#include <vector>
#include <algorithm>
#include <atomic>
#include <utility>

#include "../../include/nyxhip.h"
#include "knobs.h"
#include "roi_kernel.h"
#include "roi_radial.h"
#include "roi_outline.h"
#include "roi_caliper.h"
#include "roi_chords.h"
#include "roi_erosion.h"
#include "roi_circle.h"
#include "roi_neighbors.h"
#include "roi_morph.h"
#include "roi_hexpoly.h"
#include "roi_ih.h"
#include "roi_imq.h"
#include "roi_vol.h"

// One hipMalloc allocation, grow-only.  hipFree waits for the device's work by itself; the stream handed to reserve() states which
// work the site knows to be using the old block.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;                  // capacity
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    template <class T> T* as() const { return (T*)p; }
    explicit operator bool() const { return p != nullptr; }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
    }
    // Ensure capacity >= need.  When it must grow: synchronise `sync` (if non-null), free, allocate `want` bytes (want >= need;
    // default want == need).  On failure the buffer is empty (null, 0 bytes) and the hipError_t is returned.
    hipError_t reserve(size_t need, hipStream_t sync, size_t want = 0)
    {
        if (need <= bytes) return hipSuccess;
        hipError_t e = (p && sync) ? hipStreamSynchronize(sync) : hipSuccess;
        release();
        if (e == hipSuccess) e = hipMalloc(&p, std::max(want, need));
        if (e != hipSuccess) { p = nullptr; return e; }
        bytes = std::max(want, need);
        return hipSuccess;
    }
};

// The two buffers of a deferred list (deferred_list.h): 64 header words + the index list | the listed ROIs' per-workgroup workspace.
struct DeferredBufs { DevBuf list, ws; };

// One page-locked host block and the event of the last copy out of it: complete (both) or empty (neither).
struct PinnedSlot {
    void* p = nullptr;
    hipEvent_t done = nullptr;
    bool used = false;                 // `done` has been recorded
    PinnedSlot() = default;
    PinnedSlot(const PinnedSlot&) = delete;
    PinnedSlot& operator=(const PinnedSlot&) = delete;
    ~PinnedSlot()
    {
        if (done) (void)hipEventDestroy(done);
        if (p) (void)hipHostFree(p);
    }
    hipError_t ensure(size_t bytes)
    {
        if (p) return hipSuccess;
        if (hipError_t e = hipEventCreateWithFlags(&done, hipEventDisableTiming); e != hipSuccess) { done = nullptr; return e; }
        if (hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault); e != hipSuccess) {
            (void)hipEventDestroy(done);
            p = nullptr; done = nullptr;
            return e;
        }
        return hipSuccess;
    }
};

struct Extrema {
    uint32_t px, area, range, side;
    uint32_t vmax = 0;           // largest intensity (0: not known -- stated extrema carry none)
    bool wide_only = false;      // every ROI of the group has an intensity range beyond the counting tables (a wide-range size class)
};
struct ClassRun {              // one size class of one call, as launched (nyxhip_launch_report)
    int cls;                   // 2 * size class + (1: some ROI needs 32-bit tables); -1: the whole batch in one launch group
    uint32_t count;            // members (0xFFFFFFFF: counted on the device only)
    Extrema E;                 // extrema the carve-outs were sized for
    int workspace;             // kernel groups that ran from a global workspace instead of LDS: bit 0 INTENSITY + GLCM, 1 texture, 2 shape, 3 dependence
    hipEvent_t e0, e1;         // around the class's launches on the main stream (timing enabled), else NULL
    hipEvent_t e2 = nullptr;   // ... and the end of its launches on its workspace lane
    int cooperative = 0;       // bit 0: INTENSITY + GLCM by the several-workgroups-per-ROI kernels of roi_large.hip, bit 1: the texture families (roi_large_tex.hip), bit 2: Gabor, bit 3: bit 0's kernels on dense slides (whole-slide mode)
};
struct ClassTotals {           // sums over the members of a class (class header): what the large-ROI path sizes its workspace from
    uint64_t px, area, range1; // pixels, bounding-box cells, histogram entries (range + 1 of the members whose range the path serves)
};
struct DenseSrc {              // whole-slide mode: the dense images the next run_large call reads instead of clouds (NULL: clouds)
    const void* inten = nullptr;
    int dt = 0;                // NYXHIP_U8 | NYXHIP_U16 | NYXHIP_U32
};
constexpr int NYXHIP_INTERNAL_NEEDS_CLOUDS = -1000;   // run_class: a launch group of a window-mode call needs the materialised clouds

// nyxhip_assemble_volumes (nyxhip_volscan.hip): the assembled batch, which the context owns until the next nyxhip_assemble_volumes,
// nyxhip_release_volumes or nyxhip_destroy, and the grow-only workspaces of the scan.
struct VolScanBufs {
    DevBuf rows;                       // the batch's per-ROI arrays: volume index, label, voxel count, box origin, box, extrema | px_offset
    DevBuf cloud;                      // x | y | z | inten
    DevBuf table;                      // the label tables of a chunk | occupied slots per block; later the hits per slab of the cloud launch
    DevBuf unsorted;                   // the rows in slot order
    DevBuf sort;                       // keys and indices of the row sort (two of each), digit counts, slabs per row, block sums, slab offsets
    DevBuf stage;                      // a chunk of host volumes
    DevBuf meta;                       // VS_META_WORDS words (volscan_plan.h)
    nyxhip_batch3d batch = {};
    const uint32_t* volume_index = nullptr;
    uint32_t cap_hint = 0;             // per-volume table size that served the last call
    bool valid = false;
};

struct nyxhip_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t user_stream = nullptr;
    bool use_user_stream = false;
    DevBuf d_status;                   // int: [0] error flag of the kernels | [1] census: ROIs of <= 256 px met by the scanning form of roi_small_kernel (read with the flag)
    // census of the recent calls: how many of the ROIs were of the smallest size class.  A batch on stated extrema that mixes that class
    // with the next one runs either as two filtered whole-batch launches (nothing counted, no host round trip: right when the class is
    // rare -- the metric configuration) or through the exact class lists (right when it is common: filtered launches spend a workgroup
    // on every slot they skip).  Both give the same rows; the census only picks the cheaper one.  Host batches are counted on the host.
    uint64_t census_small = 0, census_total = 0, census_pending = 0;
    // Gabor filter bank (host-built, gabor.cpp:393-449), re-uploaded when the settings change
    DevBuf d_bank;                   // doubles
    DevBuf d_bank32;                 // the bank rounded to fp32 (Gabor screening pass)
    DevBuf d_bank16;                 // 16 x 16 banks: the band-pass filters as f16 B operands of the MFMA screening stage (ShapeArgs::gabor_bank16)
    std::vector<double> bank_key;
    uint32_t bank_zero_rows[NYXHIP_MAX_GABOR_FILTERS + 1] = {};   // ShapeArgs::gabor_zero_rows of the uploaded bank (16 x 16 kernels)
    uint32_t bank_lp_sep = 0;          // ShapeArgs::gabor_lp_sep / _B / _C of the uploaded bank
    float bank_lp_B[16] = {}, bank_lp_C[44] = {};
    uint32_t bank_box_mask = 0;                                  // ShapeArgs::gabor_box_mask of the uploaded bank
    DevBuf d_stamps;                   // diagnostic (NYXHIP_STAMPS=1 + -DNYX_STAMP build): [32] phase cycle sums
    std::string err;
    // grow-only device staging for host-memory batches
    DevBuf d_stage;
    // split GLCM: exported co-occurrence counts + matrix orders (grow-only)
    DevBuf d_glcm_ws;
    // Per-ROI words that every call clears, in ONE allocation and one hipMemsetAsync (launch_device_all): [n_roi] matrix order of every
    // ROI whose counts were exported in the CURRENT call (0: none; RoiArgs::glcm_ng) | [n_roi] pending flags of the deferred intensity
    // closing (RoiArgs::close_flag).  The second table starts at the first 256-byte boundary behind the first; the pointers of the
    // current call are glcm_ng / close_flag below (NULL: the call's mask has no use for the table).
    DevBuf d_roi_words;
    uint32_t* glcm_ng = nullptr;
    uint32_t* close_flag = nullptr;
    // deferred intensity closing (RoiArgs::close_rec): per-ROI records (grow-only)
    DevBuf d_close_rec;
    DevBuf d_logtab;                // moments: log(sqrt(d) + 0.001) per integer squared distance (roi_moments.hip)
    uint32_t logtab_n = 0;
    // contour + moments workspace (grow-only): contour points, contour lengths, per-pixel log distances
    DevBuf d_mom;
    // contour planes beyond LDS: index list (launch_contour_families); per-workgroup global scratch of every workspace launch
    DevBuf d_spill_list;
    DevBuf d_spill;
    // deferred lists of nyxhip_contour.hip, one per owner: the ROIs beyond the kernel's LDS carve, and their global workspaces
    DeferredBufs d_outline;            // roi_outline.hip: bit planes beyond LDS
    DeferredBufs d_caliper;            // roi_caliper.hip: boxes wider than the LDS column table
    DeferredBufs d_chords;             // roi_chords.hip: plane beyond LDS, or zero-intensity pixels
    DeferredBufs d_erosion;            // roi_erosion.hip: two bit planes beyond the LDS planes
    DeferredBufs d_imq;                // roi_imq.hip (nyxhip_imq.hip): intensity planes beyond the LDS plane
    DevBuf d_vol;                      // roi_vol.hip (nyxhip_vol.hip): binned boxes and sort buffers of a chunk of volumes
    // neighbor entries (roi_neighbors.hip): geometry table + candidate counts and offsets | candidate lists, minima, flags
    DevBuf d_nb_geo;
    DevBuf d_nb_cand;
    // morphology entries (roi_morph.hip): derived batch extrema | the boxes beyond the LDS column table / intensity plane and their workspace
    DevBuf d_morph_ext;
    DeferredBufs d_morph;
    // hexagonality / polygonality entries (roi_hexpoly.hip): the scratch table [n_roi x kHexpolyInLd] of the six inputs | tan(M_PI / k) of the
    // host's libm, k <= kHexpolyTanCap, filled on the context's first call
    DevBuf d_hexpoly;
    DevBuf d_hexpoly_tan;
    VolScanBufs volscan;               // nyxhip_assemble_volumes: the assembled device batch and the workspaces of the label scan
    const uint32_t* origin_x_next = nullptr;   // set by nyxhip_featurize_batch[_async]_at and the tile path for their next launch_device call:
    const uint32_t* origin_y_next = nullptr;   // device arrays [n_roi] of the ROIs' box origins (NULL: (0, 0))
    // grow-only workspaces of the fused tile path: scan tables + rows | clouds | two staging slots for host tiles
    DevBuf d_tile;
    DevBuf d_cloud;
    DevBuf d_slot[2];
    hipStream_t copy_stream = nullptr;         // H2D of the next chunk runs beside the kernels of the current one
    hipEvent_t slot_ready[2] = {nullptr, nullptr}, slot_free[2] = {nullptr, nullptr};
    // pinned staging ring of the host tile path (staged_h2d of nyxhip_tiles.hip): the library's own page-locked memory between a pageable
    // caller and the DMA engine
    static constexpr int kStageSlots = 4;
    static constexpr size_t kStageSlotBytes = (size_t)32 << 20;
    PinnedSlot h_stage[kStageSlots];
    int h_stage_next = 0;
    nyxhip::WindowSrc win_next = {};                   // set by the tile path for its next launch_device call: read ROIs from their tile windows
    DenseSrc dense_next;                       // set by launch_dense_slides around its run_large call
    uint32_t tile_cap_hint = 0;                // per-tile table size that served the last call
    // result kept for nyxhip_fetch_result() (host-memory calls with out_table == NULL): device-resident, grow-only
    //   [res_cap x res_cols] doubles | [res_cap] labels | [res_cap] tile indices
    DevBuf d_res;
    size_t res_cap = 0, res_rows = 0, res_cols = 0;
    double* res_table() const { return d_res.as<double>(); }
    uint32_t* res_label() const { return (uint32_t*)(d_res.as<char>() + (((size_t)res_cap * res_cols * 8 + 255) & ~(size_t)255)); }
    uint32_t* res_tile() const { return res_label() + res_cap; }
    // size classes of a call (launch_device_all): ROI indices grouped by class, class headers on the device and their pinned host copy
    DevBuf d_cls_list;
    DevBuf d_cls_hdr;
    PinnedSlot h_cls_hdr;               // (its event is not used)
    std::vector<ClassRun> runs;         // the classes of the last call as launched (nyxhip_launch_report)
    // large-ROI path (roi_large.hip): per-ROI blocks of histogram / plane / matrices, and the work maps + offsets + counters
    // Workspace lanes: the one-workgroup-per-ROI launches of a large class are a chain of dependent passes per ROI (milliseconds)
    // by a few hundred workgroups at most -- a fraction of the chip.  Each large class runs them on a stream of its own beside the
    // main stream (which goes on with the several-workgroups-per-ROI kernels and the LDS classes), with scratch of its own; the
    // lanes are forked from the main stream at the start of a call and joined into it at its end.
    static constexpr int kLanes = 12;              // 0-3: the large classes; 4-6: the LDS size classes of an exact call (run_class);
                                                   // 8, 10: contour + moments of a batch with boxes beyond LDS (the bulk | the big boxes);
                                                   // 9: the dependence trio of a large class; 11: Gabor of size class 2 beside the smaller classes
    static constexpr int kMomLane = 8, kDepLane = 9, kMomLaneBig = 10, kGaborLane = 11;
    hipStream_t lane_stream[kLanes] = {};
    hipEvent_t lane_done[kLanes] = {};
    hipEvent_t lane_fork = nullptr;
    DevBuf lane_buf[kLanes];
    bool lane_used[kLanes] = {};
    // ... and of the texture families (roi_large_tex.hip): one pair per lane (+ one for the main stream), the lanes run side by side
    DevBuf ltex_buf[kLanes + 1];
    DevBuf ltex_aux[kLanes + 1];
    DevBuf d_large;
    DevBuf d_large_aux;
    // timing
    int timing = 0;            // 0 off | 1 two events around every call (nyxhip_timing_get) | 2 also two events around every launch group (nyxhip_launch_report's ms)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t ev_used = 0;
    hipStream_t stream() const { return use_user_stream ? user_stream : own_stream; }
};

// Sets the origins of the context's next launch_device call and clears them on every way out of the scope.
struct OriginScope {
    nyxhip_ctx* c;
    OriginScope(nyxhip_ctx* ctx, const uint32_t* ox, const uint32_t* oy) : c(ctx) { c->origin_x_next = ox; c->origin_y_next = oy; }
    OriginScope(const OriginScope&) = delete;
    OriginScope& operator=(const OriginScope&) = delete;
    ~OriginScope() { c->origin_x_next = c->origin_y_next = nullptr; }
};

// Waits for two streams on every way out of a scope: a host pipeline must not return -- error returns included -- while copies out of
// the caller's arrays or kernels on them are in flight (the caller may free the arrays the moment the entry returns).
struct StreamDrain {
    hipStream_t a, b;
    ~StreamDrain() { (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b); }
};

// families the kernels cover so far
constexpr uint32_t kTexture = NYXHIP_FAM_GLRLM | NYXHIP_FAM_GLSZM | NYXHIP_FAM_NGTDM;
constexpr uint32_t kShape = NYXHIP_FAM_GABOR | NYXHIP_FAM_ZERNIKE;
constexpr uint32_t kDependence = NYXHIP_FAM_GLDZM | NYXHIP_FAM_GLDM | NYXHIP_FAM_NGLDM;
constexpr uint32_t kMoments = NYXHIP_FAM_SMOMS | NYXHIP_FAM_IMOMS;
constexpr uint32_t kOutline = NYXHIP_FAM_FRACTAL | NYXHIP_FAM_EULER | NYXHIP_FAM_ROI_RADIUS;   // roi_outline.hip; their columns follow the intensity block
// families that read the ROI's ordered contour (launch_contour_families)
constexpr uint32_t kCircleGeodetic = NYXHIP_FAM_CIRCLES | NYXHIP_FAM_GEODETIC;   // roi_circle.hip; their columns follow EULER_NUMBER, in front of ROI_RADIUS_MEAN
constexpr uint32_t kContourFams = kMoments | NYXHIP_FAM_RADIAL | NYXHIP_FAM_FRACTAL | NYXHIP_FAM_ROI_RADIUS | kCircleGeodetic;
constexpr uint32_t kCaliper = NYXHIP_FAM_FERET | NYXHIP_FAM_MARTIN | NYXHIP_FAM_NASSENSTEIN;   // roi_caliper.hip; their columns follow FRACT_DIM_PERIMETER
constexpr uint32_t kEllipseErosion = NYXHIP_FAM_ELLIPSE | NYXHIP_FAM_EROSION;   // roi_erosion.hip; their columns follow the intensity block, in front of kOutline's
constexpr uint32_t kBehindIntensity = kOutline | kCaliper | NYXHIP_FAM_CHORDS | kEllipseErosion | kCircleGeodetic;   // families whose columns lie between the intensity block and GLCM
constexpr uint32_t kTailFams = kContourFams | NYXHIP_FAM_EULER | kCaliper | NYXHIP_FAM_CHORDS | kEllipseErosion | kCircleGeodetic;   // ... and everything else launch_contour_families serves (no size classes)
constexpr uint32_t kImplemented = NYXHIP_FAM_INTENSITY | NYXHIP_FAM_GLCM | kTexture | kShape | kDependence | kMoments | NYXHIP_FAM_RADIAL | kOutline | kCaliper | NYXHIP_FAM_CHORDS | kEllipseErosion | kCircleGeodetic;

namespace nyxhip __attribute__((visibility("hidden"))) {

extern std::atomic<int> g_ctx_on_device[64];          // live contexts per device (default memory budgets are shared among them)

int fail(nyxhip_ctx* ctx, int code, const std::string& msg);   // records msg (ctx == NULL: for nyxhip_last_error(NULL)), returns code

#define HIP_TRY(ctx, call)                                                                    \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess)                                                                \
            return fail(ctx, NYXHIP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

// nyxhip_columns.hip
bool settings_ok(const nyxhip_settings* s, uint32_t mask, std::string& why);
// nyxhip_dispatch.hip
int use_lane(nyxhip_ctx* ctx, int lane, hipStream_t* st);   // the stream of workspace lane `lane`, forked from the call's stream on first use
uint32_t pow2ceil(uint32_t v);
int make_layout(uint32_t mask, const nyxhip_settings* s, int n_cols, uint32_t max_px, uint32_t max_area, uint32_t max_range, LdsLayout& L,
                std::string& why, size_t cap = 0, uint32_t vmax = 0, bool wide_only = false);
int ensure_stage(nyxhip_ctx* ctx, size_t bytes);
int check_status(nyxhip_ctx* ctx);
int launch_add_offset(const uint32_t* in, uint32_t add, uint32_t n, uint32_t* out, hipStream_t st);   // out[i] = in[i] + add
void clear_runs(nyxhip_ctx* ctx);
int launch_device(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px,
                  uint32_t max_area, uint32_t max_range, uint32_t max_side, bool hinted = true);
int validate(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* out, size_t ld);
int launch_dense_slides(nyxhip_ctx* ctx, const nyxhip_batch* b, const void* d_inten, int dt, uint32_t mask, const nyxhip_settings* s, double* d_out, size_t ld,
                        const Extrema& E, const ClassTotals& tot, bool* served);   // whole-slide mode: INTENSITY + GLCM of dense images (roi_large.hip)
// nyxhip_tiles.hip: what the host pipelines share (the tile path and the whole-slide path of nyxhip_slides.hip)
hipError_t staged_h2d(nyxhip_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t st);   // pageable host -> device through the pinned ring
int ensure_copy_pipeline(nyxhip_ctx* ctx);                                                          // copy_stream, slot_ready / slot_free
// nyxhip_contour.hip
int launch_contour_families(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px,
                            uint32_t max_area, uint32_t max_side, bool allow_lane, MomArgs* contour_out = nullptr);
// nyxhip_neighbors.hip: the neighbor columns of a device-resident batch -> d_out [n_roi x ld] (enqueued on the context's stream).  The rows of
// an image are given by image_offset (CSR, device) or image_id (ascending per row, device); both NULL: one image.
int neighbors_device(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* d_ox, const uint32_t* d_oy, const uint64_t* d_image_offset, uint64_t n_images,
                     const uint32_t* d_image_id, int32_t pixel_distance, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px,
                     uint32_t max_area, uint32_t max_side);
// nyxhip_ih.hip: the kIhCols intensity-histogram columns of a device-resident batch -> d_out [n_roi x ld] (enqueued on the context's stream).
// Reads px_offset, inten, min_inten, max_inten of the batch.  max_px: the largest ROI (0: not known).
int ih_settings_check(nyxhip_ctx* ctx, const nyxhip_settings* s);      // NYXHIP_ERR_UNSUPPORTED beyond kIhMaxBins
int ih_device(nyxhip_ctx* ctx, const nyxhip_batch* b, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px);
// nyxhip_imq.hip: the kImqCols image-quality columns of a device-resident batch -> d_out [n_roi x ld] (enqueued on the context's stream; the
// boxes beyond kImqLdsCells cost one read-back).  max_area: the largest box in cells (0: not known).
int imq_device(nyxhip_ctx* ctx, const nyxhip_batch* b, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_area);
int imq_check_status(nyxhip_ctx* ctx);                                 // check_status with this class's reading of NYXHIP_ERR_UNSUPPORTED
extern const char* const kImqWidthMessage;
// nyxhip_morph.hip: the columns of morphology mask `morph` of a device-resident batch -> d_out [n_roi x ld] (enqueued on the context's stream; the
// contour chain and the boxes beyond the LDS carve cost a read-back each).  d_ox / d_oy: device arrays of the box origins (NULL: (0, 0)).
// max_px / max_area / max_side: the batch extrema (any 0: derived on the device).
int morph_device(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* d_ox, const uint32_t* d_oy, uint32_t morph, const nyxhip_settings* s,
                 double* d_out, size_t ld, uint32_t max_px, uint32_t max_area, uint32_t max_side);
// The parts of neighbors_device and morph_device behind the contour chain: the same launches over a chain that has already run (`m`: the
// argument block launch_contour_families handed back).  morph_from_contours reads no contour when `morph` holds neither CONTOUR nor HULL.
int neighbors_from_contours(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* d_ox, const uint32_t* d_oy, const uint64_t* d_image_offset,
                            uint64_t n_images, const uint32_t* d_image_id, int32_t pixel_distance, const MomArgs& m, double* d_out, size_t ld);
int morph_from_contours(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* d_ox, const uint32_t* d_oy, uint32_t morph, const MomArgs& m, double* d_out,
                        size_t ld, uint32_t max_area, uint32_t max_side);
int derive_batch_extrema(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t* max_px, uint32_t* max_area, uint32_t* max_side);   // each at least 1; one read-back
// nyxhip_hexpoly.hip: the kHexpolyCols columns of HexagonalityPolygonalityFeature of a device-resident batch -> d_out [n_roi x ld] (enqueued on
// the context's stream).  Arguments as neighbors_device.  ONE contour chain feeds the neighbor kernels and roi_morph_kernel; with the
// Feret kernel they fill the context's scratch table (roi_hexpoly.h), which the closing kernel reads.
int hexpoly_device(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* d_ox, const uint32_t* d_oy, const uint64_t* d_image_offset, uint64_t n_images,
                   const uint32_t* d_image_id, int32_t pixel_distance, const nyxhip_settings* s, double* d_out, size_t ld, uint32_t max_px,
                   uint32_t max_area, uint32_t max_side);
// nyxhip_neighbors.hip: the batch entry shared by the classes that relate the ROIs of an image (neighbors_device, hexpoly_device)
using ImageBatchFn = int (*)(nyxhip_ctx*, const nyxhip_batch*, const uint32_t*, const uint32_t*, const uint64_t*, uint64_t, const uint32_t*, int32_t,
                             const nyxhip_settings*, double*, size_t, uint32_t, uint32_t, uint32_t);
int image_batch_entry(nyxhip_ctx* ctx, const nyxhip_batch* b, const uint32_t* origin_x, const uint32_t* origin_y, const uint64_t* image_offset,
                      uint64_t n_images, int32_t pixel_distance, const nyxhip_settings* s, double* out, size_t ld, int n_cols, ImageBatchFn device_fn);
int pixel_distance_check(nyxhip_ctx* ctx, int32_t pixel_distance);     // NYXHIP_ERR_INVALID_ARG at or below 0, NYXHIP_ERR_UNSUPPORTED beyond kNbMaxDistance
// What reduces the ROIs the tile path assembles to rows (tiles_run / tiles_chunk of nyxhip_tiles.hip): the family kernels, or a class with
// entries of its own.  mask: the family mask of Families, the morphology mask of Morph, else 0.  pixel_distance: of Neighbors and Hexpoly.
struct TileReducer {
    enum Kind { Families, Neighbors, Ih, Imq, Morph, Hexpoly } kind;
    uint32_t mask;
    int32_t pixel_distance;
};

} // namespace nyxhip
