/*
 * nyxhip.h -- C ABI of the MI355X-native per-ROI feature reducer.
 *
 * This is the drop-in boundary for the reference's ROI-batch reduce step:
 *
 *   reduce_trivial_rois_manual(std::vector<int>& Pending, Environment& env)
 *       /root/reference/src/nyx/reduce_trivial_rois.cpp:772-795
 *   reduce_trivial_2d(...)                       reduce_trivial_rois.cpp:62-413
 *   runParallel(F::reduce, nThr, ...)            src/nyx/parallel.h:23-42
 *
 * i.e. "given a batch of in-RAM ROIs (pixel cloud + bounding box + min/max),
 * fill every ROI's feature values for the enabled feature families".
 * The reference keeps ROIs as `LR` records (src/nyx/roi_cache.h:31-84) holding
 * an AoS `Pixel2{long x; long y; uint inten}` cloud (features/pixel.h:52-61) and a
 * dense bounding-box matrix (features/image_matrix.h:284-304); here the same
 * information crosses the boundary as flat SoA arrays (plain pointers + sizes).
 *
 * Everything below is plain C: no C++ types, no torch types.  All calls return
 * an int status (NYXHIP_OK == 0); nyxhip_last_error() gives the message.
 * Degenerate ROIs are not errors: they produce the reference's soft-NaN
 * sentinel values (reference: glcm.cpp:27-95, intensity.cpp:121-122).
 */
#ifndef NYXHIP_H
#define NYXHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NYXHIP_ABI_VERSION 2   /* 2: tile ABI v2 (nyxhip_tiles), sharded entry; every v1 symbol is kept */

/* ---- status codes ------------------------------------------------------- */
enum {
    NYXHIP_OK = 0,
    NYXHIP_ERR_INVALID_ARG = 1,   /* null pointer, bad size, bad mask          */
    NYXHIP_ERR_NO_DEVICE = 2,     /* HIP runtime / GPU not available           */
    NYXHIP_ERR_HIP = 3,           /* a HIP call failed (message has detail)    */
    NYXHIP_ERR_UNSUPPORTED = 4,   /* setting outside what the kernels cover    */
    NYXHIP_ERR_ROI_TOO_LARGE = 5, /* ROI exceeds the LDS-resident capacity     */
    NYXHIP_ERR_INTERNAL = 6       /* a device loop reached its bound (a defect) */
};

/* ---- feature families (bitmask) -----------------------------------------
 * One bit per reference FeatureMethod class on the hot path; replaces the
 * `if (F::required(fs)) runParallel(F::reduce ...)` ladder of
 * reduce_trivial_rois.cpp:65-70 (intensity), :199-204 (GLCM), :207-212 (GLRLM),
 * :223-228 (GLSZM), :247-252 (NGTDM), :364-369 (Gabor), :373-378 (Zernike). */
enum {
    NYXHIP_FAM_INTENSITY = 1u << 0, /* PixelIntensityFeatures, 36 columns      */
    NYXHIP_FAM_GLCM      = 1u << 1, /* GLCMFeature, 30*n_angles + 29 columns   */
    NYXHIP_FAM_GLRLM     = 1u << 2, /* GLRLMFeature, 16*4 + 16 columns         */
    NYXHIP_FAM_GLSZM     = 1u << 3, /* GLSZMFeature, 16 columns                */
    NYXHIP_FAM_NGTDM     = 1u << 4, /* NGTDMFeature, 5 columns                 */
    NYXHIP_FAM_GABOR     = 1u << 5, /* GaborFeature, n_gabor_filters columns   */
    NYXHIP_FAM_ZERNIKE   = 1u << 6, /* ZernikeFeature, 30 columns              */
    /* the remaining dependence / distance-zone texture families */
    NYXHIP_FAM_GLDZM     = 1u << 7, /* GLDZMFeature, 18 columns (features/gldzm.h:18-38)  */
    NYXHIP_FAM_GLDM      = 1u << 8, /* GLDMFeature, 14 columns  (features/gldm.h:30-46)   */
    NYXHIP_FAM_NGLDM     = 1u << 9, /* NGLDMfeature, 19 columns (features/ngldm.h:17-38)  */
    NYXHIP_FAM_SMOMS     = 1u << 10, /* Smoms2D_feature, 90 columns: shape moments (features/2d_geomoments.h:247-340)      */
    NYXHIP_FAM_IMOMS     = 1u << 11, /* Imoms2D_feature, 90 columns: intensity moments (features/2d_geomoments.h:99-193)   */
    /* the rest of the "low-frequency intensity distribution" block (featureset.h:352-357).  Not part of NYXHIP_FAM_ALL:
     * that constant keeps the twelve families it named before this one existed; OR this bit in explicitly.
     * Bit 12 stays unassigned: a mask that holds it is NYXHIP_ERR_INVALID_ARG, as it has always been. */
    NYXHIP_FAM_RADIAL    = 1u << 13, /* RadialDistributionFeature, 3 x 8 columns: FRAC_AT_D, MEAN_FRAC, RADIAL_CV (features/radial_distribution.h) */
    /* three classes of the shape block that need no absolute ROI position (featureset.h:46-160).  Like NYXHIP_FAM_RADIAL they are
     * not part of NYXHIP_FAM_ALL; bits 12 and 14 stay unassigned (NYXHIP_ERR_INVALID_ARG).  The columns follow the intensity block.
     * Undefined in the reference, hence here: ROI_RADIUS_* of an ROI whose merged contour is a single point. */
    NYXHIP_FAM_FRACTAL   = 1u << 15, /* FractalDimensionFeature, 2 columns: FRACT_DIM_BOXCOUNT, FRACT_DIM_PERIMETER (features/fractal_dim.h) */
    NYXHIP_FAM_EULER     = 1u << 16, /* EulerNumberFeature, 1 column: EULER_NUMBER, mode 8 (features/euler_number.h)                        */
    NYXHIP_FAM_ROI_RADIUS = 1u << 17, /* RoiRadiusFeature, 3 columns: ROI_RADIUS_MEAN, ROI_RADIUS_MAX, ROI_RADIUS_MEDIAN (features/roi_radius.h) */
    /* the three caliper classes (featureset.h:93-114, features/caliper.h): statistics of diameters of the convex hull turned in steps of
     * 10 degrees.  Not part of NYXHIP_FAM_ALL.  Their columns sit between FRACT_DIM_PERIMETER and EULER_NUMBER (enum order).  These bits,
     * NYXHIP_FAM_CHORDS and NYXHIP_FAM_CIRCLES are the only ones that read the ROI origin of nyxhip_featurize_batch_at(): the reference stores every rotated hull vertex as `float`
     * (features/rotation.cpp:37-68), so its values depend on where the ROI lies in its image.  Through the entries without an origin
     * the rows are those of an ROI whose bounding box starts at (0, 0).  An ROI of fewer than 2 pixels has no hull: all columns of
     * the requested classes are settings.soft_nan (caliper_feret.cpp:19-32). */
    NYXHIP_FAM_FERET     = 1u << 18, /* CaliperFeretFeature, 8 columns: MIN_FERET_ANGLE, MAX_FERET_ANGLE, STAT_FERET_DIAM_{MIN,MAX,MEAN,MEDIAN,STDDEV,MODE} */
    NYXHIP_FAM_MARTIN    = 1u << 19, /* CaliperMartinFeature, 6 columns: STAT_MARTIN_DIAM_{MIN,MAX,MEAN,MEDIAN,STDDEV,MODE}                                */
    NYXHIP_FAM_NASSENSTEIN = 1u << 20, /* CaliperNassensteinFeature, 6 columns: STAT_NASSENSTEIN_DIAM_{MIN,MAX,MEAN,MEDIAN,STDDEV,MODE}                    */
    /* ChordsFeature (featureset.h:116-132, features/chords.h): statistics of the chords of the pixel cloud turned in 20 steps of
     * pi / 20 about the centre of its box.  Not part of NYXHIP_FAM_ALL.  Columns between STAT_NASSENSTEIN_DIAM_MODE and EULER_NUMBER
     * (enum order).  Reads the ROI origin of nyxhip_featurize_batch_at(), like the caliper bits: the reference rounds every turned pixel
     * coordinate to float and truncates it toward zero (features/rotation.cpp:70-91), so the chords depend on where the ROI lies.
     * Reads the intensities only for "zero or not" (a zero-intensity pixel is a hole, image_matrix.cpp:206-237) and relies on
     * nyxhip_batch::min_inten to tell whether an ROI has any.  An ROI without a closed chord has 16 zeros (chords.cpp:59-60). */
    NYXHIP_FAM_CHORDS    = 1u << 21, /* 16 columns: MAXCHORDS_{MAX,MAX_ANG,MIN,MIN_ANG,MEDIAN,MEAN,MODE,STDDEV}, then the same eight for ALLCHORDS */
    /* EllipseFittingFeature (featureset.h:62-68, features/ellipse_fitting.h): Legendre's ellipse of inertia of the pixel cloud.  Not part of
     * NYXHIP_FAM_ALL.  Columns directly behind the intensity block, in front of EROSIONS_2_VANISH / FRACT_DIM_BOXCOUNT (enum order).
     * Reads coordinates only (no intensities, no origin: central moments do not move with the box); no column can be NaN. */
    NYXHIP_FAM_ELLIPSE   = 1u << 22, /* 6 columns: MAJOR_AXIS_LENGTH, MINOR_AXIS_LENGTH, ELONGATION, ECCENTRICITY, ORIENTATION, ROUNDNESS */
    /* ErosionPixelsFeature (featureset.h:85-86, features/erosion.h): erosions of the box mask by the 3 x 3 cross until nothing is left
     * (at most 1000).  Not part of NYXHIP_FAM_ALL.  Columns behind ROUNDNESS, in front of FRACT_DIM_BOXCOUNT.  Relies on
     * nyxhip_batch::min_inten / max_inten: an ROI with min_inten == max_inten is skipped, as the reference's driver does, and has 0. */
    NYXHIP_FAM_EROSION   = 1u << 23, /* 2 columns: EROSIONS_2_VANISH, EROSIONS_2_VANISH_COMPLEMENT (never assigned by the class: 0) */
    /* EnclosingInscribingCircumscribingCircleFeature (featureset.h:150-152, features/circle.h) over the ROI's merged contour.  Not part
     * of NYXHIP_FAM_ALL.  Columns directly behind EULER_NUMBER, in front of GEODETIC_LENGTH / ROI_RADIUS_MEAN (enum order).  The third
     * reader of the ROI origin of nyxhip_featurize_batch_at(): the reference searches the enclosing circle in `float` over ABSOLUTE
     * contour points and truncates midpoints to integers, so its values depend on where the ROI lies.  An ROI without a contour
     * (one pixel, two pixels, an anti-diagonal) is skipped by the class and has three zeros (circle.cpp:257). */
    NYXHIP_FAM_CIRCLES   = 1u << 24, /* 3 columns: DIAMETER_MIN_ENCLOSING_CIRCLE, DIAMETER_CIRCUMSCRIBING_CIRCLE, DIAMETER_INSCRIBING_CIRCLE */
    /* GeodeticLengthThicknessFeature (featureset.h:154-155, features/geodetic_len_thickness.h): the rectangle model over the contour's
     * perimeter and the pixel count.  Not part of NYXHIP_FAM_ALL.  Columns behind DIAMETER_INSCRIBING_CIRCLE, in front of
     * ROI_RADIUS_MEAN.  Coordinate differences only: does not read the origin.  Bits 26-31 stay unassigned (NYXHIP_ERR_INVALID_ARG). */
    NYXHIP_FAM_GEODETIC  = 1u << 25, /* 2 columns: GEODETIC_LENGTH, THICKNESS */
    NYXHIP_FAM_NORTH_STAR = 0x7Fu,  /* the seven families of BASELINE.json's north_star */
    NYXHIP_FAM_ALL       = 0xFFFu
};

#define NYXHIP_MAX_GLCM_ANGLES 4
#define NYXHIP_MAX_GABOR_FILTERS 16

/* ---- settings ------------------------------------------------------------
 * Mirrors the slots of `Fsettings` indexed by `NyxSetting`
 * (src/nyx/feature_settings.h:17-54) as filled by
 * Environment::compile_feature_settings (src/nyx/env_features.cpp:713-736),
 * plus the class-static knobs the reference keeps process-global:
 * GLCMFeature::angles / symmetric_glcm (features/glcm.cpp:8-9) and the Gabor
 * bank (features/gabor.cpp:14-25). */
typedef struct nyxhip_settings {
    double soft_nan;          /* NyxSetting::SOFTNAN  (default 0.0): written where the
                                 reference writes it AND the value reaches its table.
                                 Not so for GLCM on a ROI whose binned minimum equals
                                 its binned maximum: glcm.cpp:27-95 assigns it, save_value
                                 (:210-215) replaces it, and the row is 0.0.  INTENSITY
                                 and the moment families never write it (raw NaN stays:
                                 nyxhip_finalize_table).                             */
    double tiny;              /* NyxSetting::TINY     (default 1e-10)          */
    int32_t grey_depth;       /* NyxSetting::GREYDEPTH: >0 matlab binning with
                                 that many levels, <0 radiomics binning with
                                 |n| bins (texture_feature.h:100-102); also
                                 the intensity-histogram bin count
                                 (intensity.cpp:125)                           */
    int32_t ibsi;             /* NyxSetting::IBSI: no binning when non-zero    */
    int32_t glcm_grey_depth;  /* NyxSetting::GLCM_GREYDEPTH (degeneracy guard
                                 only, glcm.cpp:23-29)                         */
    int32_t glcm_offset;      /* NyxSetting::GLCM_OFFSET (default 1)           */
    int32_t glcm_n_angles;    /* GLCMFeature::angles.size()                    */
    int32_t glcm_angles[NYXHIP_MAX_GLCM_ANGLES]; /* subset of {0,45,90,135}    */
    int32_t glcm_symmetric;   /* GLCMFeature::symmetric_glcm                   */
    /* Gabor bank (features/gabor.cpp:14-25) */
    double gabor_gamma, gabor_sig2lam, gabor_f0lp, gabor_graythr;
    int32_t gabor_kersize;
    int32_t gabor_n_filters;
    double gabor_f0[NYXHIP_MAX_GABOR_FILTERS];
    double gabor_theta[NYXHIP_MAX_GABOR_FILTERS];   /* radians */
} nyxhip_settings;

/* Fills `s` with the reference defaults (environment.cpp / env_features.cpp:
 * SOFTNAN 0.0, TINY 1e-10, grey depth 64, IBSI off, GLCM offset 1, angles
 * {0,45,90,135}, asymmetric; Gabor gamma .1, sig2lam .8, n 16, f0LP .1,
 * thr .025, bank {(4,0),(16,pi/4),(32,pi/2),(64,3pi/4)}). */
void nyxhip_default_settings(nyxhip_settings* s);

/* ---- a batch of ROIs -------------------------------------------------------
 * SoA restatement of `std::vector<int> labels` + `unordered_map<int,LR>`
 * (the two containers `functype` receives, parallel.h:13).  ROI r owns pixels
 * [px_offset[r], px_offset[r+1]).  Coordinates are relative to the ROI's
 * bounding-box origin (LR::aabb), so they fit uint16 for every in-RAM
 * ("trivial") ROI.  Pixel order inside an ROI is the scan order of the caller
 * (column-major for the in-memory API, phase2_2d.cpp:655-656); no kernel
 * result depends on it beyond floating-point summation order -- with one
 * exception, NYXHIP_FAM_RADIAL: its centre pixel is the FIRST pixel, in this
 * order, that attains the minimum of max_sqdist - min_sqdist to the contour
 * (Pixel2::find_center, features/pixel.cpp:155 compares with a strict `<`), so
 * a row of that family depends on the pixel order through this tie-break,
 * exactly as in the reference.
 *
 * `memory` says where ALL pointers of the struct live. */
enum { NYXHIP_MEM_HOST = 0, NYXHIP_MEM_DEVICE = 1,
       /* nyxhip_tiles only: host memory AND the caller's statement that both tile arrays are mappings of their own (mmap, a
        * page-aligned allocation that is not handed back to an allocator arena while the call runs).  Their whole pages are
        * then registered for the call (hipHostRegister) and copied by DMA in place; plain NYXHIP_MEM_HOST goes through the
        * library's own pinned staging ring and assumes nothing about the caller's allocator ("Host memory"). */
       NYXHIP_MEM_HOST_OWN_MAPPING = 2 };

typedef struct nyxhip_batch {
    uint64_t n_roi;
    const uint32_t* roi_label;   /* [n_roi]   LR::label (informational)        */
    const uint64_t* px_offset;   /* [n_roi+1] CSR offsets into x/y/inten       */
    const uint16_t* x;           /* [n_px]    Pixel2::x - aabb.xmin            */
    const uint16_t* y;           /* [n_px]    Pixel2::y - aabb.ymin            */
    const uint32_t* inten;       /* [n_px]    Pixel2::inten                    */
    const uint32_t* bbox_w;      /* [n_roi]   aabb width                       */
    const uint32_t* bbox_h;      /* [n_roi]   aabb height                      */
    const uint32_t* min_inten;   /* [n_roi]   LR::aux_min                      */
    const uint32_t* max_inten;   /* [n_roi]   LR::aux_max                      */
    const double* slide_min;     /* [n_roi] or NULL: SlideProps::min_preroi_inten
                                    of the ROI's slide (intensity.cpp:72-77);
                                    NULL = slide_idx < 0 (feature left at 0)   */
    const double* slide_max;     /* [n_roi] or NULL                            */
    int32_t memory;              /* NYXHIP_MEM_HOST | NYXHIP_MEM_DEVICE        */
    /* Batch extrema, used to size the per-workgroup LDS carve-out.  The reference
     * tracks the same quantities per dataset (Dataset::dataset_max_roi_area / _w /
     * _h, src/nyx/dataset.h:12-18).  0 = unknown: the library derives them (for a
     * device batch that costs one small device->host copy and a stream sync). */
    uint32_t max_px;             /* max over ROIs of px_offset[r+1]-px_offset[r] */
    uint32_t max_bbox_area;      /* max over ROIs of bbox_w[r]*bbox_h[r]        */
    uint32_t max_inten_range;    /* max over ROIs of max_inten[r]-min_inten[r]     */
    uint32_t max_bbox_side;      /* max over ROIs of max(bbox_w[r], bbox_h[r])     */
                                 /* (all four are derived when max_px == 0)        */
} nyxhip_batch;

typedef struct nyxhip_ctx nyxhip_ctx;

/* ---- lifecycle ------------------------------------------------------------ */
int nyxhip_abi_version(void);

/* Binds a context to one GPU (one context per GPU / per process rank).  Fails
 * with NYXHIP_ERR_NO_DEVICE when no HIP device exists: there is no CPU
 * fallback behind this ABI. */
int nyxhip_init(int device, nyxhip_ctx** out_ctx);
void nyxhip_destroy(nyxhip_ctx* ctx);
const char* nyxhip_last_error(const nyxhip_ctx* ctx);

/* Launch on a caller-owned hipStream_t (e.g. torch's current stream) instead of
 * the context's own stream.  NULL restores the context stream. */
int nyxhip_set_stream(nyxhip_ctx* ctx, void* hip_stream);

/* ---- output-table layout ----------------------------------------------------
 * Columns follow `Feature2D` enum order with the angle / index expansion of
 * save_features_2_buffer (src/nyx/output_2_buffer.cpp:303-584): angled GLCM and
 * GLRLM features expand to `_0,_45,_90,_135`, GABOR to `_i`, ZERNIKE2D to `_Z i`.
 * Column names are the reference's user-facing feature names. */
int nyxhip_n_columns(uint32_t family_mask, const nyxhip_settings* s);
/* Writes the NUL-terminated name of column `col` into buf; returns NYXHIP_OK or
 * NYXHIP_ERR_INVALID_ARG. */
int nyxhip_column_name(uint32_t family_mask, const nyxhip_settings* s, int col,
                       char* buf, size_t buf_len);

/* ---- the hot path -----------------------------------------------------------
 * Replaces reduce_trivial_rois_manual() for the families in `family_mask`.
 * out_table is row-major [n_roi x out_ld] doubles (out_ld >= n_columns), in host
 * memory when batch->memory == NYXHIP_MEM_HOST, in device memory otherwise.
 * Synchronous: results are complete on return.  NaN/inf are NOT replaced here;
 * that is the table writer's job in the reference too (force_finite_number,
 * helpers/helpers.h:376-382) -- see nyxhip_finalize_table(). */
int nyxhip_featurize_batch(nyxhip_ctx* ctx, const nyxhip_batch* batch,
                           uint32_t family_mask, const nyxhip_settings* s,
                           double* out_table, size_t out_ld);

/* Asynchronous form for device-resident batches: enqueues the kernels on the
 * context's stream and returns; call nyxhip_sync() (or synchronise the stream
 * given to nyxhip_set_stream) before reading out_table. */
int nyxhip_featurize_batch_async(nyxhip_ctx* ctx, const nyxhip_batch* batch,
                                 uint32_t family_mask, const nyxhip_settings* s,
                                 double* out_table, size_t out_ld);
int nyxhip_sync(nyxhip_ctx* ctx);

/* The two calls above with the ROIs' positions: origin_x[r] / origin_y[r] = aabb.xmin / aabb.ymin of ROI r in its image ([n_roi],
 * in the memory of the batch's other pointers, batch->memory).  Both NULL = every origin (0, 0): exactly nyxhip_featurize_batch
 * [_async].  Only NYXHIP_FAM_FERET / _MARTIN / _NASSENSTEIN / _CHORDS / _CIRCLES read the origin; every other column is the same with and without it. */
int nyxhip_featurize_batch_at(nyxhip_ctx* ctx, const nyxhip_batch* batch, const uint32_t* origin_x, const uint32_t* origin_y,
                              uint32_t family_mask, const nyxhip_settings* s, double* out_table, size_t out_ld);
int nyxhip_featurize_batch_async_at(nyxhip_ctx* ctx, const nyxhip_batch* batch, const uint32_t* origin_x, const uint32_t* origin_y,
                                    uint32_t family_mask, const nyxhip_settings* s, double* out_table, size_t out_ld);

/* Host-side NaN/inf -> soft_nan replacement over a host table, as
 * save_features_2_buffer does per value (output_2_buffer.cpp:296,...). */
void nyxhip_finalize_table(double* table, size_t n_rows, size_t n_cols, size_t ld,
                           double soft_nan);

/* ---- fused tile path ("next" row: phases 1-2 + reduce on the device) ---------
 * Replaces gatherRoisMetricsInMemory (src/nyx/phase1.cpp:373-409) +
 * scanTrivialRoisInMemory (src/nyx/phase2_2d.cpp:637-684) +
 * allocateTrivialRoisBuffers (:427-465) + the RAM batching of
 * processTrivialRoisInMemory (:686-770) + reduce_trivial_rois_manual for a stack
 * of equally sized intensity/label tile pairs in device or host memory.
 *
 * Tile t occupies rows [t*height, (t+1)*height) of one tall image.  Labels are
 * per tile and may be ANY non-zero 32-bit values (the reference keys ROIs through
 * hash containers, roi_cache.h / phase1.cpp:373-409): nothing is sized by label
 * magnitude.  Rows come back ordered by (tile, label) -- images in input order,
 * labels ascending, the row order of the reference's table
 * (workflow_pythonapi.cpp:140-182 + output_2_buffer.cpp:305-306).
 *
 * Tiles keep the caller's unsigned element type (the reference casts everything to
 * uint32 on the host, nyxus.py:486-489; here the cast happens in the kernels, so
 * H2D carries the image's own bytes). */
enum { NYXHIP_U8 = 1, NYXHIP_U16 = 2, NYXHIP_U32 = 4 };   /* element size in bytes */

/* Slide min / max behind COVERED_IMAGE_INTENSITY_RANGE (intensity.cpp:72-77):
 * MONTAGE  = the in-memory API: the montage prescan leaves them at +/-DBL_MAX
 *            (slideprops.cpp:27-28,74-75), the feature is range / -inf = -0.0;
 * PER_TILE = one tile is one slide: min / max of the intensities under any mask
 *            (scan_slide_props, slideprops.cpp:456-...), computed on the device;
 * GIVEN    = per-tile values from the caller (a slide cut into several tiles). */
enum { NYXHIP_SLIDE_MONTAGE = 0, NYXHIP_SLIDE_PER_TILE = 1, NYXHIP_SLIDE_GIVEN = 2 };

typedef struct nyxhip_tiles {
    const void* inten;          /* [n_tiles][height][width] of inten_dtype             */
    const void* label;          /* [n_tiles][height][width] of label_dtype, 0 = no ROI */
    int32_t inten_dtype;        /* NYXHIP_U8 | NYXHIP_U16 | NYXHIP_U32                 */
    int32_t label_dtype;
    uint32_t width, height, n_tiles;
    int32_t memory;             /* NYXHIP_MEM_HOST | NYXHIP_MEM_DEVICE (tiles AND outputs) */
    int32_t slide_mode;         /* NYXHIP_SLIDE_*                                      */
    const double* slide_min;    /* host [n_tiles], NYXHIP_SLIDE_GIVEN only             */
    const double* slide_max;
    uint64_t max_device_bytes;  /* device workspace budget of the call -- the counterpart of the
                                   reference's ram_limit batching (phase2_2d.cpp:694-705): the stack
                                   is processed in chunks of tiles that fit; 0 = half of the free
                                   device memory                                       */
} nyxhip_tiles;

/* Host tiles: chunk c+1 is copied to the device while chunk c is being reduced (two device
 * staging slots, copies and kernels on different streams).
 * Outputs (host memory when tiles->memory == NYXHIP_MEM_HOST, else device memory):
 * out_labels / out_tile_index (may be NULL) / out_table hold up to max_rows rows.  When the
 * stack has more ROIs, NYXHIP_ERR_INVALID_ARG is returned and *n_roi_out holds the count.
 * Host memory only: out_table == NULL asks the library to keep the result in the context;
 * *n_roi_out then sizes the caller's buffers for nyxhip_fetch_result(). */
int nyxhip_featurize_tiles_v2(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, uint32_t family_mask,
                              const nyxhip_settings* s, uint32_t* out_labels, uint32_t* out_tile_index,
                              uint64_t max_rows, double* out_table, size_t out_ld, uint64_t* n_roi_out);
/* Copies the result kept by the last nyxhip_featurize_tiles_v2(out_table == NULL) call and frees it. */
int nyxhip_fetch_result(nyxhip_ctx* ctx, uint32_t* out_labels, uint32_t* out_tile_index,
                        double* out_table, size_t out_ld);

/* One node, several GPUs: the stack (HOST memory) is block-partitioned over the contexts
 * (context g gets tiles [g*n/G, (g+1)*n/G) -- ROIs are independent, the label vector is
 * already sliced like this by the reference's runParallel, parallel.h:34-41), each context
 * is driven by its own host thread, and the rows are returned in stack order as above.
 * Contexts may sit on the same or on different devices.  out_table == NULL: see
 * nyxhip_fetch_result_sharded(). */
int nyxhip_featurize_tiles_sharded(nyxhip_ctx* const* ctxs, int n_ctx, const nyxhip_tiles* tiles,
                                   uint32_t family_mask, const nyxhip_settings* s,
                                   uint32_t* out_labels, uint32_t* out_tile_index, uint64_t max_rows,
                                   double* out_table, size_t out_ld, uint64_t* n_roi_out);
/* out_table == NULL above keeps every context's rows in the context; this copies them out in
 * stack order (sum of the counts = the *n_roi_out of that call) and frees them. */
int nyxhip_fetch_result_sharded(nyxhip_ctx* const* ctxs, int n_ctx, uint32_t* out_labels,
                                uint32_t* out_tile_index, double* out_table, size_t out_ld);

/* v1 entry points (uint32 tiles, montage slide semantics).  `max_label` is only validated:
 * a label above it is NYXHIP_ERR_INVALID_ARG; pass 0xFFFFFFFF to accept every value. */
int nyxhip_featurize_tile(nyxhip_ctx* ctx, const uint32_t* inten, const uint32_t* label,
                          uint32_t width, uint32_t height, int32_t memory,
                          uint32_t max_label, uint32_t family_mask,
                          const nyxhip_settings* s,
                          uint32_t* out_labels, uint64_t max_rows,
                          double* out_table, size_t out_ld, uint64_t* n_roi_out);
int nyxhip_featurize_tiles(nyxhip_ctx* ctx, const uint32_t* inten, const uint32_t* label,
                           uint32_t width, uint32_t height, uint32_t n_tiles, int32_t memory,
                           uint32_t max_label, uint32_t family_mask, const nyxhip_settings* s,
                           uint32_t* out_labels, uint32_t* out_tile_index, uint64_t max_rows,
                           double* out_table, size_t out_ld, uint64_t* n_roi_out);

/* ---- the neighbor class -------------------------------------------------------
 * NeighborsFeature (features/neighbors.cpp:125-536, featureset.h:162-171): NUM_NEIGHBORS, PERCENT_TOUCHING, CLOSEST_NEIGHBOR1_DIST,
 * CLOSEST_NEIGHBOR1_ANG, CLOSEST_NEIGHBOR2_DIST, CLOSEST_NEIGHBOR2_ANG, ANG_BW_NEIGHBORS_MEAN, ANG_BW_NEIGHBORS_STDDEV,
 * ANG_BW_NEIGHBORS_MODE.  No per-ROI reduction: it relates the ROIs of ONE image to each other (boxes that overlap at pixel_distance,
 * then exact distances between the merged contours), so it claims no family bit and has entries and an output table
 * [n_roi x NYXHIP_NEIGHBOR_COLS] of its own; nyxhip_n_columns / nyxhip_column_name do not know it.  ROIs of different images are never
 * neighbors.  Every value is finite (soft_nan never shows): an ROI without a neighbor has zeros.
 * pixel_distance <= 0 is NYXHIP_ERR_INVALID_ARG; beyond 46340 its square overflows the reference's int: NYXHIP_ERR_UNSUPPORTED. */
#define NYXHIP_NEIGHBOR_COLS 9
int nyxhip_neighbor_column_name(int col, char* buf, size_t buf_len);

/* A batch of ROIs of n_images images: image k owns rows [image_offset[k], image_offset[k + 1]) (CSR, [n_images + 1], in batch->memory
 * like the origins; NULL: one image).  The rows of an image must be strictly ascending in roi_label (the reference walks its labels
 * sorted, and the order decides ties): anything else is NYXHIP_ERR_INVALID_ARG.  origin_x / origin_y as in nyxhip_featurize_batch_at
 * (both NULL: every origin (0, 0)).  Reads roi_label, px_offset, x, y, inten, bbox_w, bbox_h of the batch.  Synchronous. */
int nyxhip_neighbors_batch(nyxhip_ctx* ctx, const nyxhip_batch* batch, const uint32_t* origin_x, const uint32_t* origin_y,
                           const uint64_t* image_offset, uint64_t n_images, int32_t pixel_distance,
                           const nyxhip_settings* s, double* out_table /* [n_roi x 9] */, size_t out_ld);
/* The tile path (label scan, ROI assembly, chunks under max_device_bytes) with one image per tile; rows in the (tile, label) order of
 * nyxhip_featurize_tiles_v2, outputs as there. */
int nyxhip_neighbors_tiles(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, int32_t pixel_distance, const nyxhip_settings* s,
                           uint32_t* out_labels, uint32_t* out_tile_index, uint64_t max_rows,
                           double* out_table, size_t out_ld, uint64_t* n_roi_out);

/* ---- the IBSI intensity-histogram class ------------------------------------------
 * IntensityHistogramFeatures (features/intensity_histogram.cpp:29-325, featureset.h:584-637): the 46 codes IH_MEAN_VAL .. IH_BIN_SIZE, all
 * derived from one N-bin histogram over the ROI's [min_inten, max_inten], N = settings.grey_depth.  The codes lie at the very end of
 * Feature2D and every bit of the family mask is spoken for, so the class has entries and an output table [n_roi x NYXHIP_IH_COLS] of its
 * own, like the neighbor class; nyxhip_n_columns / nyxhip_column_name do not know it.  The class gates itself: with settings.ibsi == 0,
 * grey_depth < 2 (a negative, i.e. radiomics, grey depth lands here), max_inten <= min_inten or an empty ROI, all 46 values of the row
 * are settings.soft_nan.  Every column has the reference's bits except IH_ENTROPY_VAL / IH_ENTROPY_IDX, which go through log() and
 * agree to rounding.  NaN / inf are not replaced (nyxhip_finalize_table), as in every other table.  Integer images only: the reference's
 * float_domain_map is the identity unless the slide is a float image or HU mode is on, and neither exists behind this ABI.
 * ibsi != 0 with grey_depth > 4096 is NYXHIP_ERR_UNSUPPORTED: the bin counters live in LDS. */
#define NYXHIP_IH_COLS 46
int nyxhip_ih_column_name(int col, char* buf, size_t buf_len);

/* Reads px_offset, inten, min_inten, max_inten of the batch and nothing else (host or device memory, like nyxhip_neighbors_batch;
 * batch->max_px is a hint as everywhere).  Synchronous. */
int nyxhip_ih_batch(nyxhip_ctx* ctx, const nyxhip_batch* batch, const nyxhip_settings* s,
                    double* out_table /* [n_roi x 46] */, size_t out_ld);
/* The tile path (label scan, ROI assembly, chunks under max_device_bytes) with this class as the reducer; rows in the (tile, label)
 * order of nyxhip_featurize_tiles_v2, outputs as there. */
int nyxhip_ih_tiles(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, const nyxhip_settings* s,
                    uint32_t* out_labels, uint32_t* out_tile_index, uint64_t max_rows,
                    double* out_table, size_t out_ld, uint64_t* n_roi_out);

/* ---- whole-slide mode ---------------------------------------------------------------
 * The reference's second mode (featurize_files(files, None, single_roi = True), featurize_directory() without a label directory;
 * workflow_2d_whole.cpp:36-213, reduce_trivial_rois.cpp:798-819, slideprops.cpp:101-254): every slide is ONE ROI with label 1 that
 * covers the whole image, zero-valued pixels included.  Area = width * height, the box is the image with origin (0, 0), aux_min /
 * aux_max are the extrema over all pixels, and the slide extrema are the same two values (COVERED_IMAGE_INTENSITY_RANGE = range / range).
 *
 * `slides` is the struct of the tile path: inten [n_tiles][height][width] of inten_dtype, memory NYXHIP_MEM_HOST or NYXHIP_MEM_DEVICE
 * (the images AND out_table), max_device_bytes as there.  `label` must be NULL (NYXHIP_ERR_INVALID_ARG otherwise); label_dtype,
 * slide_mode, slide_min and slide_max are not read.  One row per slide, in input order, nyxhip_n_columns(family_mask, s) columns in the
 * order and under the names of every other entry.  Row t has the bits of nyxhip_featurize_batch on the one-ROI batch whose cloud is
 * the slide's pixels in row-major order (x = i % width, y = i / width, intensity widened to 32 bits), bbox_w = width, bbox_h = height,
 * min_inten / max_inten the slide's extrema and slide_min / slide_max the same extrema as doubles.
 *
 * Served: any non-empty subset of bits 0-9 (NYXHIP_FAM_ALL without the two moment classes, which weight differently in this mode:
 * 2d_geomoments_basic.cpp:122-123).  Any other valid family bit is NYXHIP_ERR_UNSUPPORTED; a bit that is invalid everywhere stays
 * NYXHIP_ERR_INVALID_ARG.  width or height of 0 or above 65534 is NYXHIP_ERR_UNSUPPORTED (coordinates inside an ROI are 16-bit);
 * n_tiles == 0 is NYXHIP_OK and writes nothing; a single slide that does not fit max_device_bytes is NYXHIP_ERR_ROI_TOO_LARGE.  The
 * stack is processed in chunks of slides that fit the budget; host chunks travel through the pinned staging ring of the tile path, the
 * copy of chunk c + 1 beside the reduce of chunk c.  Every family keeps the limits it has behind nyxhip_featurize_batch.  Synchronous. */
int nyxhip_featurize_slides(nyxhip_ctx* ctx, const nyxhip_tiles* slides, uint32_t family_mask,
                            const nyxhip_settings* s, double* out_table, size_t out_ld);

/* ---- whole-slide mode: the rest of the *WHOLESLIDE* group ------------------------------
 * The reference's feature group for this mode (env_features.cpp:219-234) names twelve classes.  Nine are family bits 0-9 above; the
 * other three -- ContourFeature, the two moment classes and RadialDistributionFeature -- mean something else in this mode than behind
 * nyxhip_featurize_batch, so they have an entry, a mask space and a table of their own, and the entries above keep refusing them.
 * The ROI is the whole image at origin (0, 0), zero pixels included, in row-major order, and its contour is the four corners
 * K = (0,0), (w-1,0), (w-1,h-1), (0,h-1), each with the slide's maximum as intensity (features/contour.cpp:917-933):
 *   NYXHIP_WS_CONTOUR  ContourFeature::calculate over K: PERIMETER, DIAMETER_EQUAL_PERIMETER, EDGE_MEAN_INTENSITY, EDGE_STDDEV_INTENSITY,
 *                      EDGE_MAX_INTENSITY, EDGE_MIN_INTENSITY, EDGE_INTEGRATED_INTENSITY (the reference's bits)
 *   NYXHIP_WS_SMOMS / NYXHIP_WS_IMOMS  the 90 columns each of NYXHIP_FAM_SMOMS / NYXHIP_FAM_IMOMS.  The unweighted sets are those of the
 *                      batch path.  In the weighted sets a pixel of the first / last row or column weighs epsilon = 0.001 whatever its
 *                      intensity; every other pixel weighs I * log(d + epsilon), d = min(x, w-1-x, y, h-1-y) (the reference's
 *                      dist_to_segment to the four sides, 2d_geomoments_basic.cpp:58-96), I = the intensity (IMOMS) or 1 (SMOMS).
 *   NYXHIP_WS_RADIAL   the 24 columns of NYXHIP_FAM_RADIAL: find_center by the reference's hill descent over the FOUR points (its first
 *                      step is 2: corners 0 and 2 decide whether 1 and 3 are looked at), the first pixel in row-major order wins ties;
 *                      bins, wedges and tail as behind NYXHIP_FAM_RADIAL.  A 1 x 1 slide (max_sqdist == 0, undefined in the reference)
 *                      has 24 zeros.  The block is ALWAYS computed against K: the reference's omission of the contour when no contour or
 *                      moment code is requested (reduce_trivial_rois.cpp:446-457) is the caller's to mirror.
 * Blocks stand in the order of the bits; names are those of nyxhip_morph_column_name(NYXHIP_MORPH_CONTOUR) and of nyxhip_column_name for
 * the family bit alone.  The contract is nyxhip_imq_slides': label must be NULL, U8 / U16 / U32 in host or device memory (the images AND
 * out_table), chunks under max_device_bytes through the staging ring, one row per slide in input order, n_tiles == 0 is NYXHIP_OK, a side
 * of 0 or above 65534 is NYXHIP_ERR_UNSUPPORTED, a slide beyond the budget NYXHIP_ERR_ROI_TOO_LARGE, a zero mask or a bit above 8
 * NYXHIP_ERR_INVALID_ARG (nyxhip_wsgroup_n_columns: -1).  NaN / inf are not replaced (nyxhip_finalize_table).  Synchronous.
 * The image is read in place: once for the maximum (CONTOUR), once for the moments and the centre, once for the radial bins.  Sums are
 * added in an order fixed by the slide's shape, so a row has the same bits whatever shares its call, its chunk or its place in the stack. */
#define NYXHIP_WS_CONTOUR 1u   /*  7 */
#define NYXHIP_WS_SMOMS   2u   /* 90 */
#define NYXHIP_WS_IMOMS   4u   /* 90 */
#define NYXHIP_WS_RADIAL  8u   /* 24 */
int nyxhip_wsgroup_n_columns(uint32_t ws_mask);
int nyxhip_wsgroup_column_name(uint32_t ws_mask, int col, char* buf, size_t buf_len);
int nyxhip_wsgroup_slides(nyxhip_ctx* ctx, const nyxhip_tiles* slides, uint32_t ws_mask,
                          const nyxhip_settings* s, double* out_table, size_t out_ld);

/* ---- image quality: focus score and saturation ---------------------------------------
 * Four of the six codes of the reference's FeatureIMQ (featureset.h:920-931), the classes behind its ImageQuality Python class
 * (reduce_trivial_rois.cpp:388-412, :631-654): FocusScoreFeature (features/focus_score.cpp:188-282) and SaturationFeature
 * (features/saturation.cpp:74-95).  They live in an enum of their own, so the class has entries and an output table
 * [n_roi x NYXHIP_IMQ_COLS] of its own, like the neighbor and intensity-histogram classes; nyxhip_n_columns / nyxhip_column_name do not
 * know it.  Columns, in enum order: FOCUS_SCORE, LOCAL_FOCUS_SCORE, MAX_SATURATION, MIN_SATURATION.
 *
 * Everything is taken over the ROI's dense plane P (bbox_h rows, bbox_w columns): the intensity at every cloud pixel and 0 at every
 * other cell of the box (LR::aux_image_matrix) -- the background takes part.  With n = bbox_w * bbox_h and
 * L = P[y-1][x] + P[y+1][x] + P[y][x-1] + P[y][x+1] - 4 P[y][x] (cells outside the plane are 0):
 *   FOCUS_SCORE        the population variance of L over all n cells
 *   LOCAL_FOCUS_SCORE  tiles of M = bbox_h / 2 rows and N = bbox_w / 2 columns at (y0, x0), y0 in {0, M, ..} while y0 < bbox_h - M and
 *                      x0 likewise (the reference's loop bound, as it is): each tile's own Laplacian (zeros outside the TILE) and
 *                      population variance; the sum of the tile variances / 4.  A box with a side of 1 makes the reference's loop
 *                      run for ever: settings.soft_nan here, the other three columns as defined.
 *   MAX_SATURATION     #(P == max P) / n
 *   MIN_SATURATION     #(P == min P) / n, and 0 when min P == max P.  An ROI that does not fill its box has min P = 0.
 * An ROI without pixels or with an empty box has four times settings.soft_nan.  NaN / inf are not replaced (nyxhip_finalize_table).
 * The two saturation columns have the reference's bits.  The sums behind the focus columns are exact integers (the sum of L in 64 bits,
 * of L^2 in 128), so they agree with the reference's fp64 sums to rounding, and a row has the same bits whatever shares its call.
 * WIDTH: the 64-bit sum of L cannot overflow while 4 * max_inten * n < 2^63.  An ROI (or slide) beyond that bound is
 * NYXHIP_ERR_UNSUPPORTED; nothing wraps silently.
 * NOT SERVED, and why:
 *   POWER_SPECTRUM_SLOPE  features/power_spectrum.cpp:168-175 bins every FFT output by floor(sqrt(value)) + 1 -- the value, not its
 *                         radius -- and :85-90 index raw_radii (max(rows, cols) entries) with indices up to the padded size: a
 *                         discontinuous function of floating-point FFT outputs with an out-of-bounds read, which no tolerance pins.
 *   SHARPNESS             features/sharpness.cpp:200-205 "transposes back" with a sequential in-place swap loop: the identity for a
 *                         square box, a shape-dependent scramble for any other, w * h dependent steps per ROI; vetted against nothing. */
#define NYXHIP_IMQ_COLS 4
int nyxhip_imq_column_name(int col, char* buf, size_t buf_len);

/* Reads px_offset, x, y, inten, bbox_w, bbox_h, min_inten, max_inten of the batch (host or device memory, like nyxhip_ih_batch;
 * batch->max_px / max_bbox_area are hints as everywhere).  min_inten / max_inten must be the cloud's extrema.  Synchronous. */
int nyxhip_imq_batch(nyxhip_ctx* ctx, const nyxhip_batch* batch, const nyxhip_settings* s,
                     double* out_table /* [n_roi x 4] */, size_t out_ld);
/* The tile path (label scan, ROI assembly, chunks under max_device_bytes) with these classes as the reducer; rows in the (tile, label)
 * order of nyxhip_featurize_tiles_v2, outputs as there. */
int nyxhip_imq_tiles(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, const nyxhip_settings* s,
                     uint32_t* out_labels, uint32_t* out_tile_index, uint64_t max_rows,
                     double* out_table, size_t out_ld, uint64_t* n_roi_out);
/* Whole-slide mode under the contract of nyxhip_featurize_slides: `label` must be NULL, inten_dtype U8 / U16 / U32, chunks under
 * max_device_bytes, one row per slide, n_tiles == 0 is NYXHIP_OK, a side of 0 or above 65534 is NYXHIP_ERR_UNSUPPORTED.  The slides are
 * read in place (no cloud, no plane).  Row t has the bits of nyxhip_imq_batch on the equivalent one-ROI batch. */
int nyxhip_imq_slides(nyxhip_ctx* ctx, const nyxhip_tiles* slides, const nyxhip_settings* s,
                      double* out_table, size_t out_ld);

/* ---- volumes (3-D): voxel intensity and 3-D GLCM -------------------------------
 * The first two classes of the reference's `Feature3D` enum (featureset.h:643-797), behind entries and a family mask of their own:
 * the 2-D mask, nyxhip_n_columns and nyxhip_column_name do not know them.
 *   NYXHIP_VFAM_INTENSITY   D3_VoxelIntensityFeatures (features/3d_intensity.cpp:45-183): the 36 codes 3COV .. 3UNIFORMITY_PIU
 *   NYXHIP_VFAM_GLCM        D3_GLCM_feature (features/3d_glcm.cpp): 30 angled codes over the 13 directions of shifts[] (:16-31) and
 *                           the 29 _AVE codes save_value assigns (:147-175)
 * Any other bit of a volume mask is NYXHIP_ERR_INVALID_ARG.
 *
 * COLUMNS.  The intensity block first (36 columns, Feature3D order, the reference's user-facing names: "3COV" ..), then the GLCM block:
 * every angled code in Feature3D order (3GLCM_ACOR, 3GLCM_ASM, 3GLCM_CLUPROM ..) as 13 columns "<name>_<k>", k = 0 .. 12 the index
 * into shifts[] = (dx, dy, dz): (1,1,1) (1,1,0) (1,1,-1) (1,0,1) (1,0,0) (1,0,-1) (1,-1,1) (1,-1,0) (1,-1,-1) (0,1,1) (0,1,0) (0,1,-1)
 * (0,0,1); then the 29 _AVE codes in Feature3D order (3GLCM_ASM_AVE .. 3GLCM_SUMVARIANCE_AVE), one column each.  3GLCM_HOM2 has no _AVE
 * code in the enum; every _AVE code the enum holds is assigned (the line 3d_glcm.cpp:176 repeats, commented out, what :170 assigns).
 * An _AVE value is std::reduce over the 13 directional values / 13 (texture_feature.h:121-130), blank directions (soft_nan) included.
 *
 * SETTINGS, read with the meaning the 3-D classes give them:
 *   grey_depth       |grey_depth| = bin count of the intensity block's histogram (3d_intensity.cpp:115)
 *   ibsi             GLCM: no binning, levels are the intensities
 *   glcm_grey_depth  GLCM binning (3d_glcm.cpp:51): > 0 matlab binning with that many levels, < 0 radiomics binning with |n| bins
 *   glcm_offset      D3_GLCM_feature::offset, the class static (3d_glcm.cpp:8).  The reference's GLCM_OFFSET setting does not reach the
 *                    3-D class (nothing assigns the static from it): a caller that mirrors the reference passes 1.  Must be >= 1.
 *   glcm_symmetric   D3_GLCM_feature::symmetric_glcm, the class static (:9, read at :368); radiomics and IBSI binning count
 *                    symmetrically whatever it says
 *   soft_nan         the 30 values of a direction whose matrix is blank (:184-218), and every value of an ROI without voxels
 *   glcm_n_angles / glcm_angles, tiny and the Gabor fields are not read.
 * LIMITS.  A box side is at most 65534; a box holds at most NYXHIP_VOL_MAX_CELLS = 2^24 cells (256^3: the pair counts and the exact
 * integer numerators of the closing formulas are 32-bit) and an ROI at most 2^32 - 1 voxels: beyond, NYXHIP_ERR_ROI_TOO_LARGE.  The
 * co-occurrence matrix lives in LDS: more than NYXHIP_VOL_GLCM_MAX_LEVELS levels (|glcm_grey_depth|, or the largest intensity in IBSI
 * mode) is NYXHIP_ERR_UNSUPPORTED, never a wrong row.  A voxel outside its box is never stored: NYXHIP_ERR_INVALID_ARG.
 * Every row has the same bits whatever shares its call, chunk, memory kind or batch order. */
enum {
    NYXHIP_VFAM_INTENSITY = 1u << 0,
    NYXHIP_VFAM_GLCM = 1u << 1,
    NYXHIP_VFAM_ALL = 0x3
};
#define NYXHIP_VOL_GLCM_DIRECTIONS 13
#define NYXHIP_VOL_GLCM_MAX_LEVELS 128
#define NYXHIP_VOL_MAX_CELLS (1u << 24)

/* SoA restatement of LR::raw_pixels_3D + LR::aux_image_cube, shaped like nyxhip_batch.  ROI r owns voxels
 * [px_offset[r], px_offset[r+1]); coordinates are relative to the origin of the ROI's box. */
typedef struct nyxhip_batch3d {
    uint64_t n_roi;
    const uint32_t* roi_label;   /* [n_roi]   LR::label (informational, may be NULL) */
    const uint64_t* px_offset;   /* [n_roi+1] CSR offsets into x/y/z/inten     */
    const uint16_t* x;           /* [n_px]    Pixel3::x - box origin           */
    const uint16_t* y;
    const uint16_t* z;
    const uint32_t* inten;       /* [n_px]    Pixel3::inten                    */
    const uint32_t* bbox_w;      /* [n_roi]   aux_image_cube width  (x)        */
    const uint32_t* bbox_h;      /* [n_roi]   ... height (y)                   */
    const uint32_t* bbox_d;      /* [n_roi]   ... depth  (z)                   */
    const uint32_t* min_inten;   /* [n_roi]   LR::aux_min                      */
    const uint32_t* max_inten;   /* [n_roi]   LR::aux_max                      */
    const double* slide_min;     /* [n_roi] or NULL: slide_idx < 0, 3COVERED_IMAGE_INTENSITY_RANGE = 1 (3d_intensity.cpp:58-65) */
    const double* slide_max;     /* [n_roi] or NULL                            */
    int32_t memory;              /* NYXHIP_MEM_HOST | NYXHIP_MEM_DEVICE: where ALL pointers live */
    /* Stated extrema; all three are derived when max_px == 0 (a device batch then costs one device->host copy of the boxes). */
    uint32_t max_px;             /* max over ROIs of the voxel count           */
    uint32_t max_bbox_cells;     /* max over ROIs of bbox_w * bbox_h * bbox_d  */
    uint32_t max_inten_range;    /* max over ROIs of max_inten - min_inten     */
    uint64_t max_device_bytes;   /* device workspace budget of the call (binned boxes, sort buffers); the ROIs run in chunks that
                                    fit it.  0 = half of the free device memory.  One ROI that does not fit: NYXHIP_ERR_ROI_TOO_LARGE. */
} nyxhip_batch3d;

/* Column catalogue of a volume mask: the count (< 0: invalid mask) and the name of column `col`. */
int nyxhip_vol_n_columns(uint32_t vol_mask, const nyxhip_settings* s);
int nyxhip_vol_column_name(uint32_t vol_mask, const nyxhip_settings* s, int col, char* buf, size_t buf_len);

/* One row of nyxhip_vol_n_columns(vol_mask, s) values per ROI.  Host batch: host table.  Device batch: device table.  Synchronous.
 * NaN / inf are not replaced (nyxhip_finalize_table). */
int nyxhip_featurize_volumes(nyxhip_ctx* ctx, const nyxhip_batch3d* batch, uint32_t vol_mask, const nyxhip_settings* s,
                             double* out_table, size_t out_ld);

/* ---- volumes (3-D): GLDM, NGLDM and NGTDM -----------------------------------
 * Three more classes of the reference's Feature3D enum on the batch type of the volume entries, behind entries and a mask space of their
 * own (the volume mask keeps its two bits):
 *   NYXHIP_VTEX_GLDM    D3_GLDM_feature (features/3d_gldm.cpp): 14 codes 3GLDM_SDE .. 3GLDM_LDHGLE.  26 shifts, a voxel counts itself.
 *   NYXHIP_VTEX_NGLDM   D3_NGLDM_feature (features/3d_ngldm.cpp): 19 codes 3NGLDM_LDE .. 3NGLDM_DCENE (3NGLDM_DCP before 3NGLDM_GLM, as in
 *                       the enum).  24 shifts (none straight up or down), over every interior cell of the box, off-ROI cells included.
 *   NYXHIP_VTEX_NGTDM   D3_NGTDM_feature (features/3d_ngtdm.cpp): 5 codes 3NGTDM_COARSENESS .. 3NGTDM_STRENGTH over the cube of Chebyshev
 *                       radius ngtdm_radius, background cells summed too.
 * The blocks of a row stand in that order.  SETTINGS READ.  nyxhip_settings: ibsi, soft_nan, grey_depth (NGLDM: to_grayscale(v, 0,
 * max_inten, grey_depth) on every cell of the box; the value is read as unsigned, as the reference's parameter is, so a negative one
 * exceeds the level cap).  nyxhip_voltex_settings: the three slots below; GLDM and NGTDM bin with greyInfo = ibsi ? 0 : <class>_grey_depth
 * (> 0 matlab levels, < 0 radiomics bins, 0 none).  The reference starts all three at 0 (env_features.cpp:712-736).
 * soft_nan is written where the classes assign it: a flat ROI (GLDM, NGLDM), no dependence zone (GLDM), fewer than two levels (NGTDM);
 * and in every column of an ROI without voxels.  Other NaN / inf stay (nyxhip_finalize_table).  ngtdm_radius == 0 is legal: no voxel has
 * a neighbour, every code is NaN (soft_nan with fewer than two levels), and the level cap does not apply to the NGTDM block.
 * A cloud names each cell of its box at most once.
 * LIMITS.  Those of the volume entries (side, NYXHIP_VOL_MAX_CELLS, stated extrema, max_device_bytes, voxels outside their box), and:
 * the level tables live in LDS, so more than NYXHIP_VOLTEX_MAX_LEVELS levels is NYXHIP_ERR_UNSUPPORTED, never a wrong row --
 * |gldm_grey_depth|, |ngtdm_grey_depth| and grey_depth are checked on the host, the largest intensity of an ROI (IBSI mode, or a grey
 * depth of 0) on the device; ngtdm_radius outside 0 .. NYXHIP_VOLTEX_MAX_RADIUS is NYXHIP_ERR_UNSUPPORTED.
 * Every sum that more than one thread adds to is an integer: a row has the same bits whatever shares its call, chunk, memory kind or
 * batch order. */
enum {
    NYXHIP_VTEX_GLDM = 1u << 0,
    NYXHIP_VTEX_NGLDM = 1u << 1,
    NYXHIP_VTEX_NGTDM = 1u << 2,
    NYXHIP_VTEX_ALL = 0x7
};
#define NYXHIP_VOLTEX_MAX_LEVELS 128
#define NYXHIP_VOLTEX_MAX_RADIUS 3
typedef struct nyxhip_voltex_settings {
    int32_t gldm_grey_depth;     /* NyxSetting::GLDM_GREYDEPTH of fsett_D3_GLDM   */
    int32_t ngtdm_grey_depth;    /* NyxSetting::NGTDM_GREYDEPTH of fsett_D3_NGTDM */
    int32_t ngtdm_radius;        /* NyxSetting::NGTDM_RADIUS: Chebyshev radius of the cube gather_zones scans */
} nyxhip_voltex_settings;

/* Column catalogue of a texture mask: the count (< 0: invalid mask, 0 or any foreign bit) and the name of column `col`. */
int nyxhip_voltex_n_columns(uint32_t tex_mask);
int nyxhip_voltex_column_name(uint32_t tex_mask, int col, char* buf, size_t buf_len);

/* One row of nyxhip_voltex_n_columns(tex_mask) values per ROI.  Host batch: host table.  Device batch: device table.  Synchronous. */
int nyxhip_featurize_volumes_tex(nyxhip_ctx* ctx, const nyxhip_batch3d* batch, uint32_t tex_mask, const nyxhip_settings* s,
                                 const nyxhip_voltex_settings* t, double* out_table, size_t out_ld);

/* ---- volumes (3-D): GLRLM and GLSZM -------------------------------------------
 * Two more classes of the reference's Feature3D enum on the batch type of the volume entries, behind entries and a mask space of their
 * own (the volume mask and the texture mask keep their bits):
 *   NYXHIP_VZONE_GLRLM   D3_GLRLM_feature (features/3d_glrlm.cpp): 16 angled codes 3GLRLM_SRE .. 3GLRLM_LRHGLE, 13 columns <name>_<k> each,
 *                        k the index into shifts13[] (3d_glrlm.cpp:17-32, fields dz, dy, dx: direction 0 is (1, 1, 1), 4 is +z, 10 is +y,
 *                        12 is +x), then the 16 codes 3GLRLM_SRE_AVE .. 3GLRLM_LRHGLE_AVE: calc_ave over the 13 values, soft_nan values
 *                        included.  224 columns.  A run is a maximal line of cells of one non-zero level along the direction; under
 *                        matlab binning the background of the box has level 1 and forms runs.
 *   NYXHIP_VZONE_GLSZM   D3_GLSZM_feature (features/3d_glszm.cpp): 16 codes 3GLSZM_SAE .. 3GLSZM_LAHGLE.  A zone is a 26-connected component
 *                        of cells of one level; cells of the background level (1 under matlab binning, else 0) form none.
 * The GLRLM block of a row stands first.  SETTINGS READ.  nyxhip_settings: ibsi, soft_nan.  nyxhip_volzone_settings: the two slots below;
 * a class bins with greyInfo = ibsi ? 0 : <class>_grey_depth (> 0 matlab levels, < 0 radiomics bins, 0 none).  The reference starts both
 * at 0.  soft_nan is written in every column of a flat ROI (min_inten == max_inten: both classes answer before they bin; an _AVE column is
 * then the average of thirteen soft_nan), of an ROI without voxels, and in the GLSZM block of an ROI without a zone.  An empty run matrix
 * gives 0 in every GLRLM column.  Other NaN / inf stay (nyxhip_finalize_table).
 * LIMITS.  Those of the volume entries (side, NYXHIP_VOL_MAX_CELLS, stated extrema, max_device_bytes, voxels outside their box), and:
 * more than NYXHIP_VOLZONE_MAX_LEVELS levels is NYXHIP_ERR_UNSUPPORTED, never a wrong row -- |glrlm_grey_depth| and |glszm_grey_depth|
 * are checked on the host, the largest intensity of an ROI (IBSI mode, or a grey depth of 0) on the device.  The workspace holds, per ROI
 * of a chunk, 8 bytes per cell of the largest box for the GLSZM labels and, for GLRLM, a table of levels x run lengths per direction
 * sized by the largest box sides of the batch (read from the boxes: a device batch costs one device->host copy of them).
 * WHERE THE REFERENCE IS UNDEFINED.  Its formulas square a run length or a zone size j as `int`: double(j * j) overflows above 46340
 * cells (3GLRLM_SRE, _LRE, _SRHGLE, _LRLGLE; 3GLSZM_SAE, _LAE: 3d_glszm.cpp:685, :709), and inten * inten * j * j of 3GLRLM_SRLGLE and
 * _LRHGLE is a 32-bit unsigned product that wraps once level x j reaches 2^16.  A box of 36 x 36 x 37 cells already holds a zone above
 * 46340 cells, so real volumes meet this.  This library computes double(j) * double(j), which is exact, everywhere.
 * Every sum that more than one thread adds to is an integer and the list of large zones is sorted before it is read: a row has the same
 * bits whatever shares its call, chunk, memory kind or batch order.  No kernel waits for another workgroup; every device loop has a
 * bound derived from the box, and one that reaches it makes the call return NYXHIP_ERR_INTERNAL. */
enum {
    NYXHIP_VZONE_GLRLM = 1u << 0,
    NYXHIP_VZONE_GLSZM = 1u << 1,
    NYXHIP_VZONE_ALL = 0x3
};
#define NYXHIP_VOLZONE_MAX_LEVELS 128
typedef struct nyxhip_volzone_settings {
    int32_t glrlm_grey_depth;    /* NyxSetting::GLRLM_GREYDEPTH of fsett_D3_GLRLM */
    int32_t glszm_grey_depth;    /* NyxSetting::GLSZM_GREYDEPTH of fsett_D3_GLSZM */
} nyxhip_volzone_settings;

/* Column catalogue of a zone mask: the count (< 0: invalid mask, 0 or any foreign bit) and the name of column `col`. */
int nyxhip_volzone_n_columns(uint32_t zone_mask);
int nyxhip_volzone_column_name(uint32_t zone_mask, int col, char* buf, size_t buf_len);

/* One row of nyxhip_volzone_n_columns(zone_mask) values per ROI.  Host batch: host table.  Device batch: device table.  Synchronous. */
int nyxhip_featurize_volumes_zones(nyxhip_ctx* ctx, const nyxhip_batch3d* batch, uint32_t zone_mask, const nyxhip_settings* s,
                                   const nyxhip_volzone_settings* t, double* out_table, size_t out_ld);

/* ---- volumes (3-D): GLDZM ----------------------------------------------------
 * The last texture class of the reference's Feature3D enum, behind an entry and a mask space of its own (the volume, texture and zone
 * masks keep their bits):
 *   NYXHIP_VDZ_GLDZM   D3_GLDZM_feature (features/3d_gldzm.cpp): 18 codes 3GLDZM_SDE .. 3GLDZM_ZDE in save_value order (GLE is computed
 *                      and not saved).
 * THE RULING.  Semantics are those of the text of 3d_gldzm.cpp, quirks included, with one exception: a cell of level 0 is treated in
 * every binning mode as the reference treats it in IBSI mode -- it forms no zone and it is always a border.  Every sum of the
 * reference's calc_features skips level 0 already and a level-0 zone adds only empty columns, so the value equals the reference's
 * wherever the reference is defined; it is not defined under radiomics binning (grey_depth < 0) for a box that holds a level-0 cell (a
 * cell outside the cloud, or a voxel of intensity 0): there it writes outside its matrix and its distances depend on traversal order.
 *   binning    greyInfo = ibsi ? 0 : grey_depth of nyxhip_settings (the class has no grey depth of its own): > 0 matlab levels -- the
 *              background of the box is then level 1, forms zones and merges with level-1 voxels, and only the box faces are borders;
 *              < 0 radiomics bins; 0 none.
 *   zones      6-connected components of equal level (E, S, W, N, +z, -z): diagonal contact does not join.
 *   distance   of a cell: in its own z-plane, along +-x and +-y, the distance to the nearest cell that is level 0 or lies on the box face
 *              (a cell on that face: 0), plus 1, the minimum of the four.  A face cell has 1, a cell beside a level-0 cell 2, and so has
 *              a cell at x == 1.  The metric of a zone is the minimum over its cells; the matrix is [level][metric - 1].
 *   ZP         Ns / voxels of the cloud; background zones under matlab binning count in Ns.  ZDE uses log2(p / Ns + 2.2e-16).
 * SETTINGS READ.  nyxhip_settings: ibsi, grey_depth, soft_nan.  soft_nan is written in all 18 columns of a flat ROI (min_inten ==
 * max_inten, before any binning) and of an ROI without voxels.  Other NaN / inf stay (nyxhip_finalize_table).
 * LIMITS.  Those of the volume entries (side, NYXHIP_VOL_MAX_CELLS, stated extrema, max_device_bytes, voxels outside their box), and:
 * more than NYXHIP_VOLDZONE_MAX_LEVELS levels is NYXHIP_ERR_UNSUPPORTED, never a wrong row -- |grey_depth| is checked on the host, the
 * largest intensity of an ROI (IBSI mode, or a grey depth of 0) on the device.  The workspace holds, per ROI of a chunk, 11 bytes per
 * cell of the largest box (level, 16-bit distance, label, zone minimum) and a table of levels x (min(w, h) / 2 + 2) sized by the
 * largest boxes of the batch (read from the boxes: a device batch costs one device->host copy of them).
 * Every sum that more than one thread adds to is an integer: a row has the same bits whatever shares its call, chunk, memory kind or
 * batch order.  No kernel waits for another workgroup; every device loop has a bound derived from the box, and one that reaches it
 * makes the call return NYXHIP_ERR_INTERNAL. */
enum {
    NYXHIP_VDZ_GLDZM = 1u << 0
};
#define NYXHIP_VOLDZONE_MAX_LEVELS 128

/* Column catalogue of a distance-zone mask: the count (< 0: invalid mask, 0 or any foreign bit) and the name of column `col`. */
int nyxhip_voldzone_n_columns(uint32_t dzone_mask);
int nyxhip_voldzone_column_name(uint32_t dzone_mask, int col, char* buf, size_t buf_len);

/* One row of 18 values per ROI.  Host batch: host table.  Device batch: device table.  Synchronous. */
int nyxhip_featurize_volumes_dzones(nyxhip_ctx* ctx, const nyxhip_batch3d* batch, uint32_t dzone_mask, const nyxhip_settings* s,
                                    double* out_table, size_t out_ld);

/* ---- volumes (3-D): shape ------------------------------------------------------
 * The shape class of the reference's Feature3D enum, behind an entry and a mask space of its own (the other four masks keep their bits):
 *   NYXHIP_VSHAPE_MORPHOLOGY   D3_SurfaceFeature (features/3d_surface.cpp:322-516): 14 codes 3AREA .. 3FLATNESS in enum order.
 * The reference's single-ROI mode (:331-352) is not served.
 *   3VOXEL_VOLUME     voxels x (4/3 pi / 8) / 0.5236; every voxel of the cloud counts, intensity 0 included.
 *   3AREA             the exposed voxel faces: per voxel the 6-neighbours that are not in the cloud.  An integer, exact.
 *   3AREA_2_VOLUME, 3COMPACTNESS1, 3COMPACTNESS2, 3SPHERICAL_DISPROPORTION, 3SPHERICITY   the reference's closed forms of those two.
 *   3MAJOR_AXIS_LEN, 3MINOR_AXIS_LEN, 3LEAST_AXIS_LEN   4 sqrt(lambda_i) of the sample covariance (divisor N - 1) of the voxel
 *                     coordinates, eigenvalues descending; 3ELONGATION, 3FLATNESS: sqrt(l1 / l0), sqrt(l2 / l0).  The covariance comes
 *                     from exact integer sums, the eigenvalues from cyclic Jacobi in fp64.  A negative eigenvalue, or one below 2^-40 of
 *                     the largest, is 0 (a rank-deficient cloud: a line, a plane); one voxel, or l0 == 0, gives 0 in all five columns.
 *   3VOLUME_CONVEXHULL = 3MESH_VOLUME
 * THE RULING.  The hull columns hold the EXACT volume of the convex hull of the centres of the voxels of non-zero intensity, and 0
 * where those span fewer than three dimensions.  The reference hulls the per-plane contours of the same voxels with a float
 * quickhull (eps 1e-10f) that is not exact: it equals this value wherever its hull is correct and is off by up to percents on round
 * or sparse clouds.  6 V is accumulated as an integer with exact integer predicates: a row has the same bits
 * whatever shares its call, chunk, memory kind or batch order.
 * SETTINGS READ.  nyxhip_settings: soft_nan, written in all 14 columns of an ROI without voxels.  No grey depth, no level cap.
 * LIMITS.  Those of the volume entries (side, NYXHIP_VOL_MAX_CELLS cells and voxels, stated extrema, max_device_bytes, voxels outside
 * their box).  The workspace holds, per ROI of a chunk, a byte per cell of the largest box and 200 to 340 bytes per (z, y) row of the
 * largest box sides of the batch (row extremes, chains, hull candidates, visited edges, edge stack).  No kernel waits for another
 * workgroup; every loop of the hull has a bound derived from its candidate count, and one that reaches it makes the call return
 * NYXHIP_ERR_INTERNAL. */
enum {
    NYXHIP_VSHAPE_MORPHOLOGY = 1u << 0
};

/* Column catalogue of a shape mask: the count (< 0: invalid mask, 0 or any foreign bit) and the name of column `col`. */
int nyxhip_vshape_n_columns(uint32_t shape_mask);
int nyxhip_vshape_column_name(uint32_t shape_mask, int col, char* buf, size_t buf_len);

/* One row of 14 values per ROI.  Host batch: host table.  Device batch: device table.  Synchronous. */
int nyxhip_featurize_volumes_shape(nyxhip_ctx* ctx, const nyxhip_batch3d* batch, uint32_t shape_mask, const nyxhip_settings* s,
                                   double* out_table, size_t out_ld);

/* ---- volumes (3-D): the label scan on the device ------------------------------
 * The step in front of the five volume entries: a stack of intensity / label volumes -> the nyxhip_batch3d of its ROIs, assembled on the
 * device (the 3-D counterpart of the label scan inside nyxhip_featurize_tiles_v2).
 *
 * ROWS.  One ROI per (volume, non-zero label value), in (volume, ascending label) order: the same label in two volumes makes two ROIs.
 * The box is the tight bounding box of the label's voxels, coordinates are relative to its corner, the voxels of an ROI stand in raster
 * order (z, then y, then x).  Voxels of intensity 0 under a label are included.  min_inten / max_inten are taken over the ROI's voxels.
 * Labels are any non-zero value of the label type: nothing is sized by the label magnitude.
 *
 * out_batch is a DEVICE batch (memory == NYXHIP_MEM_DEVICE, every pointer filled, slide_min / slide_max NULL, max_device_bytes copied from
 * `v`) that the CONTEXT owns: it stays valid until the next nyxhip_assemble_volumes (a refused one too), nyxhip_release_volumes or
 * nyxhip_destroy on the context and can be passed unchanged to any of the five volume entries with a device table.  The stated extrema max_px,
 * max_bbox_cells (saturating at 2^32 - 1; the entries refuse such boxes themselves) and max_inten_range are filled exactly.
 * out_volume_index (may be NULL) receives a device array [n_roi]: the volume of every row.  A stack without any label is NYXHIP_OK with
 * n_roi == 0 and NULL arrays.  Synchronous.
 *
 * LIMITS, checked before anything is launched where that is possible; none gives a wrong row.  NULL ctx / v / out_batch / inten / label,
 * an unknown dtype or memory kind, a zero side or n_volumes: NYXHIP_ERR_INVALID_ARG.  A side above 65534: NYXHIP_ERR_ROI_TOO_LARGE.
 * width * height * depth >= 2^32: NYXHIP_ERR_UNSUPPORTED.  One volume that does not fit max_device_bytes with its label table:
 * NYXHIP_ERR_ROI_TOO_LARGE.  More than 2^24 labels in one volume, or more than 2^31 - 1 ROIs in the stack: NYXHIP_ERR_UNSUPPORTED. */
typedef struct nyxhip_volumes {
    const void* inten;            /* [n_volumes][depth][height][width] of inten_dtype            */
    const void* label;            /* same shape, label_dtype; 0 = no ROI                          */
    int32_t inten_dtype, label_dtype;      /* NYXHIP_U8 | NYXHIP_U16 | NYXHIP_U32               */
    uint32_t width, height, depth, n_volumes;
    int32_t memory;               /* NYXHIP_MEM_HOST | NYXHIP_MEM_DEVICE: where inten / label live */
    uint64_t max_device_bytes;    /* staging + scan workspace budget; 0 = half of free device memory */
} nyxhip_volumes;

int nyxhip_assemble_volumes(nyxhip_ctx* ctx, const nyxhip_volumes* v, nyxhip_batch3d* out_batch,
                            const uint32_t** out_volume_index /* device [n_roi], may be NULL */);
/* Host copies of the labels and volume indices of the assembled batch (either may be NULL); max_rows < n_roi: NYXHIP_ERR_INVALID_ARG. */
int nyxhip_assembled_rows(nyxhip_ctx* ctx, uint32_t* out_labels, uint32_t* out_volume_index, uint64_t max_rows);
/* Frees the assembled batch and the workspaces of the scan. */
int nyxhip_release_volumes(nyxhip_ctx* ctx);

/* ---- 2-D morphology: basic morphology, contour, convex hull, extrema -------------------
 * Four classes of the reference's 2-D shape block (featureset.h:46-60, :71-82, :136-143), 41 columns:
 *   NYXHIP_MORPH_BASIC    BasicMorphologyFeatures (features/basic_morphology.cpp:19-92): AREA_PIXELS_COUNT, AREA_UM2, CENTROID_X,
 *                         CENTROID_Y, WEIGHTED_CENTROID_Y, WEIGHTED_CENTROID_X, MASS_DISPLACEMENT, COMPACTNESS, BBOX_YMIN, BBOX_XMIN,
 *                         BBOX_HEIGHT, BBOX_WIDTH, DIAMETER_EQUAL_AREA, EXTENT, ASPECT_RATIO
 *   NYXHIP_MORPH_CONTOUR  ContourFeature (features/contour.cpp:935-1021): PERIMETER, DIAMETER_EQUAL_PERIMETER, EDGE_MEAN_INTENSITY,
 *                         EDGE_STDDEV_INTENSITY, EDGE_MAX_INTENSITY, EDGE_MIN_INTENSITY, EDGE_INTEGRATED_INTENSITY
 *   NYXHIP_MORPH_HULL     ConvexHullFeature (features/convex_hull_nontriv.cpp:53-66): CIRCULARITY, CONVEX_HULL_AREA, SOLIDITY.  It reads
 *                         the perimeter, so the contour chain runs whether or not NYXHIP_MORPH_CONTOUR is set.
 *   NYXHIP_MORPH_EXTREMA  ExtremaFeature (features/extrema.cpp:15-74): EXTREMA_P1_X, EXTREMA_P1_Y .. EXTREMA_P8_X, EXTREMA_P8_Y
 * The codes lie inside the shape block, where every bit of the family mask is spoken for, so the classes have a mask space, entries
 * and an output table [n_roi x nyxhip_morph_n_columns(mask)] of their own, like the neighbor class; nyxhip_n_columns /
 * nyxhip_column_name do not know them.  The columns of a mask stand in enum order, which is the order above.
 *
 * POSITION.  BBOX_XMIN / BBOX_YMIN, CENTROID_*, WEIGHTED_CENTROID_* and the sixteen extrema columns are image coordinates: the
 * origin plus the coordinate inside the box.  MASS_DISPLACEMENT and COMPACTNESS are formed from those rounded centroids, as the
 * reference forms them, so their last bits move with the origin (by a few ulp of the coordinate).  Every other column reads
 * coordinate differences only and has the same bits wherever the ROI lies.  The boxes of a batch are tight (bbox_w - 1 and
 * bbox_h - 1 occur as coordinates), as everywhere.  A pixel outside its box is never stored: NYXHIP_ERR_INVALID_ARG.
 * AREA_UM2 is 0: the class writes it only when the XY resolution setting is positive, and the reference's feature settings
 * (env_features.cpp:712-736) never carry one, so its API always reports the member's initial 0.
 * No ROI is skipped for flat intensities (has_bad_data() is false in this version of the reference, roi_cache.cpp:43-47).
 * SUMS.  sum x, sum y, sum x I, sum y I and sum I are exact integers on the device (sum x I as two 64-bit sums over the halves of
 * the intensity); each is converted once and divided once.  That is the reference's sequential fp64 sum bit for bit while that sum
 * stays below 2^53, and the correctly rounded exact value beyond.  The weighted centroids are 0 when sum I = 0.  MASS_DISPLACEMENT is
 * sqrt(dx * dx + dy * dy), unfused.  COMPACTNESS is the standard deviation (n - 1; 0 for n <= 2, moments.h:38) of the pixel-to-centroid
 * distances divided by n: a centred second pass where the reference updates on line, so it agrees to rounding.
 * PERIMETER has the reference's bits (terms added one after the other in its order); 0 without a contour, like the five EDGE_*
 * columns.  EDGE_* run over the merged contour, every point once per time it stands there, with the cloud's intensity at the point:
 * MIN, MAX and INTEGRATED_INTENSITY are integers, MEAN is the integer sum divided by the count, STDDEV is sqrt(M2 / (count - 1)) from
 * a centred second pass (0 for count <= 2); MEAN and STDDEV agree with the reference's on-line update to rounding.
 * CONVEX_HULL_AREA = |shoelace| / 2 + (sum over hull edges of gcd(|dx|, |dy|)) / 2 + 1 over the reference's monotone-chain hull, formed
 * as one integer and converted once: exact.  Fewer than two pixels: an empty hull, area 1.  SOLIDITY = n / area.  CIRCULARITY =
 * sqrt(4 pi n / (p * p)) in IEEE operations: +inf where the perimeter is 0 -- left raw like every other table (nyxhip_finalize_table).
 * EXTREMA.  P1 / P2: the top row's leftmost / rightmost pixel; P3 / P4: the right column's top / bottom pixel; P5 / P6: the bottom
 * row's rightmost / leftmost pixel; P7 / P8: the left column's bottom / top pixel.
 * An empty ROI has zeros.  settings->soft_nan is the only field of the settings that is read (by nyxhip_finalize_table, not here).
 * LIMITS.  Those of the batch type.  A contour point outside its box makes the call return NYXHIP_ERR_INTERNAL. */
enum {
    NYXHIP_MORPH_BASIC = 1u << 0,     /* 15 columns */
    NYXHIP_MORPH_CONTOUR = 1u << 1,   /*  7 */
    NYXHIP_MORPH_HULL = 1u << 2,      /*  3: CIRCULARITY, CONVEX_HULL_AREA, SOLIDITY */
    NYXHIP_MORPH_EXTREMA = 1u << 3,   /* 16 */
    NYXHIP_MORPH_ALL = 0xFu           /* any other bit: NYXHIP_ERR_INVALID_ARG */
};

/* Column catalogue of a morphology mask: the count (< 0: invalid mask, 0 or any foreign bit) and the name of column `col`. */
int nyxhip_morph_n_columns(uint32_t morph_mask);
int nyxhip_morph_column_name(uint32_t morph_mask, int col, char* buf, size_t buf_len);

/* A batch of ROIs, host or device memory like nyxhip_neighbors_batch (a host batch is staged into one slab; out_table lives where the
 * batch lives).  origin_x / origin_y as in nyxhip_featurize_batch_at: both NULL (every origin (0, 0)) or both given, in batch->memory.
 * The extrema hints of a device batch are taken when all are stated and derived otherwise.  Reads px_offset, x, y, inten, bbox_w, bbox_h.
 * An empty batch is NYXHIP_OK.  Synchronous. */
int nyxhip_morph_batch(nyxhip_ctx* ctx, const nyxhip_batch* batch, const uint32_t* origin_x, const uint32_t* origin_y,
                       uint32_t morph_mask, const nyxhip_settings* s, double* out_table, size_t out_ld);
/* The tile path (label scan, ROI assembly, chunks under max_device_bytes) with these classes as the reducer: the origins are the
 * boxes' places inside their tile; rows in the (tile, label) order of nyxhip_featurize_tiles_v2, outputs as there. */
int nyxhip_morph_tiles(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, uint32_t morph_mask, const nyxhip_settings* s,
                       uint32_t* out_labels, uint32_t* out_tile_index, uint64_t max_rows,
                       double* out_table, size_t out_ld, uint64_t* n_roi_out);

/* ---- 2-D morphology: hexagonality and polygonality ---------------------------------------
 * HexagonalityPolygonalityFeature (features/hexagonality_polygonality.cpp:14-217, featureset.h:146-148): POLYGONALITY_AVE,
 * HEXAGONALITY_AVE, HEXAGONALITY_STDDEV -- the three codes that complete ConvexHullFeature::featureset (convex_hull.h:12-20) and with
 * it the group *ALL_MORPHOLOGY*.  A closing formula over six numbers of the ROI: the pixel count (aux_area), NUM_NEIGHBORS at
 * pixel_distance, PERIMETER, CONVEX_HULL_AREA, STAT_FERET_DIAM_MIN and STAT_FERET_DIAM_MAX.  Because it reads the neighbor count it
 * relates the ROIs of ONE image, so it has entries and an output table [n_roi x NYXHIP_HEXPOLY_COLS] of its own with the arguments of
 * the neighbor entries; nyxhip_n_columns / nyxhip_column_name do not know it.  One call runs the contour chain once and lets the
 * neighbor kernels, the morphology kernel (CONTOUR | HULL) and the Feret kernel write into a scratch table of the context, then a
 * lane per ROI closes the formula.
 * GATES, in the reference's order (:202, then :43-49 and :159).  A row is three times -1.0 (the class's `novalue`; raw, not soft_nan)
 * when the ROI has no contour, when CONVEX_HULL_AREA == 0, or when NUM_NEIGHBORS < 3.  No ROI is skipped for flat intensities
 * (has_bad_data() is false in this version of the reference, roi_cache.cpp:43-47).
 * FORMULA.  calculate() operation for operation (:34-152): the 11 areas and 14 perimeters in its order, the 55 + 91 ratios
 * 1 - |1 - a / b| in its ib < ic order summed one after the other, area ratios that are not finite left out (:91), perimeter ratios
 * not (:136: a NaN or an infinity -- STAT_FERET_DIAM_MIN == 0, a perimeter of 0 -- goes through the sums as it does there), population
 * deviations from a second pass.  Left raw like every other table (nyxhip_finalize_table).
 * BITS.  Every operation is an IEEE fp64 +, -, *, / or square root, unfused (the reference is built without FMA), and the six inputs
 * have the reference's bits, so a row whose NUM_NEIGHBORS is at most 128 has the reference's bits: tan(M_PI / k), the only
 * transcendental (:51-52), comes for k <= 128 from a table the context fills once with the host's libm.  Beyond 128 neighbors the
 * device's tan serves POLYGONALITY_AVE (the project's standing tolerance); the two hexagonality columns do not read it.
 * pixel_distance <= 0 is NYXHIP_ERR_INVALID_ARG; beyond 46340: NYXHIP_ERR_UNSUPPORTED (the neighbor class).  settings->soft_nan is
 * the only field of the settings that is read (a ROI of fewer than two pixels has it as its Feret diameters; the first gate takes
 * that row). */
#define NYXHIP_HEXPOLY_COLS 3
int nyxhip_hexpoly_column_name(int col, char* buf, size_t buf_len);

/* Arguments, memory kinds, checks and error codes of nyxhip_neighbors_batch: image k owns rows [image_offset[k], image_offset[k + 1])
 * (NULL: one image), strictly ascending in roi_label; origins both NULL or both given.  An empty batch is NYXHIP_OK.  Synchronous. */
int nyxhip_hexpoly_batch(nyxhip_ctx* ctx, const nyxhip_batch* batch, const uint32_t* origin_x, const uint32_t* origin_y,
                         const uint64_t* image_offset, uint64_t n_images, int32_t pixel_distance,
                         const nyxhip_settings* s, double* out_table /* [n_roi x 3] */, size_t out_ld);
/* The tile path (label scan, ROI assembly, chunks under max_device_bytes) with one image per tile, as nyxhip_neighbors_tiles; rows in
 * the (tile, label) order of nyxhip_featurize_tiles_v2, outputs as there. */
int nyxhip_hexpoly_tiles(nyxhip_ctx* ctx, const nyxhip_tiles* tiles, int32_t pixel_distance, const nyxhip_settings* s,
                         uint32_t* out_labels, uint32_t* out_tile_index, uint64_t max_rows,
                         double* out_table, size_t out_ld, uint64_t* n_roi_out);

/* ---- measurement hooks -------------------------------------------------------
 * Average device time (ms) per featurize call since the last nyxhip_timing_reset(),
 * measured with hipEvents recorded on the launch stream around EVERYTHING the call
 * enqueues (all kernel groups, the moments pair, the large-ROI passes).  Used by
 * bench.py for `roofline.achieved`.  on = 1: those two events per call; on = 2: also two
 * events around every launch group of the call (the "ms" of nyxhip_launch_report) -- each
 * recorded event is a marker packet on the stream, a handful of microseconds of device
 * time, so the per-group level is for diagnosis, not for the timed region of a benchmark. */
int nyxhip_timing_enable(nyxhip_ctx* ctx, int on);
int nyxhip_timing_reset(nyxhip_ctx* ctx);
int nyxhip_timing_get(nyxhip_ctx* ctx, double* avg_kernel_ms, uint64_t* n_launches);

/* The size classes of the LAST nyxhip_featurize_batch[_async] call on this context, as launched: a JSON array written to
 * buf (NUL-terminated, truncated to buf_len), one object per launch group:
 *   {"class": c, "size_class": 0..4, "wide_range": 0|1, "rois": n, "max_px": .., "max_bbox_area": .., "max_range": ..,
 *    "max_side": .., "workspace": <bit mask>, "cooperative": <bit mask>, "ms": t, "lane_ms": t2}
 * "class" < 0 = a launch over the whole batch, enqueued without counting anything because the stated batch extrema rule out
 * all but the two smallest size classes and wide intensity ranges (-1: texture + dependence kernels, -2: feature kernels,
 * -4 / -5: one-wave / four-wave shape kernels; "rois" is then the batch size); "workspace" 0 = kernels
 * with their state in LDS, else the kernel groups that run from the global workspace (bit 0 INTENSITY + GLCM, 1 texture,
 * 2 shape, 3 dependence); "cooperative" = families of the class served by several workgroups per ROI (ROIs beyond LDS): bit 0 INTENSITY +
 * GLCM, bit 1 GLRLM + GLSZM + NGTDM, bit 2 Gabor, bit 3 (with bit 0, nyxhip_featurize_slides only) the members were dense slides read in place, no clouds;
 * "ms" = device time of the class's launches on the call's stream and "lane_ms" = fork-to-end time of the class's workspace
 * launches on their own stream (large classes run them beside the main stream; null otherwise) when
 * nyxhip_timing_enable(ctx, 2) was in force for the call (waits for them), else null.  Counterpart in the
 * reference: none -- its worker threads take ROIs of any size (parallel.h:23-42); here a launch is sized by its largest
 * ROI, so a call is split by ROI size.  Returns the number of bytes the full text needs (excluding the NUL), or < 0. */
int nyxhip_launch_report(nyxhip_ctx* ctx, char* buf, size_t buf_len);

/* Diagnostic: the per-ROI words that every featurize call clears at its start, as the LAST call on this context left them -- waits for
 * the context's stream, then counts the non-zero entries among the first n_roi of each table: *n_orders the matrix orders that the
 * feature kernels stated for the GLCM feature launch (ROIs whose co-occurrence counts were exported), *n_flags the pending flags of the
 * deferred intensity closing.  A flag is raised by the feature kernel and cleared by the closing launch that consumes it, so after a
 * completed call *n_flags is 0; a table the last call's mask had no use for counts 0.  Either pointer may be NULL. */
int nyxhip_debug_roi_words(nyxhip_ctx* ctx, uint64_t n_roi, uint64_t* n_orders, uint64_t* n_flags);

#ifdef __cplusplus
}
#endif
#endif /* NYXHIP_H */
