// nyxhip_volscan.hip -- the device label scan for volumes of include/nyxhip.h: nyxhip_assemble_volumes, nyxhip_assembled_rows,
// nyxhip_release_volumes.  The kernels are in vol_assembly.hip, the arithmetic of the workspaces in volscan_plan.h.
//
// A call runs in two passes over chunks of whole volumes that fit the budget with their label tables:
//   pass 1, per chunk   host volumes: one host-to-device copy of the chunk through the pinned ring; the scan; one read-back of the meta
//                       words (overflow flag, occupied slots) -- an overflow replaces the tables by kVsCapGrow times larger ones and scans
//                       the chunk again --; the occupied slots appended to the unsorted rows.
//   between             the rows of the whole stack sorted by (volume, label), the sorted rows, extrema and offsets, one read-back of the
//                       totals, the clouds allocated.
//   pass 2, per chunk   the clouds of the chunk's rows from the chunk's volumes.
// A stack of one chunk -- every device stack whose tables fit, every host stack that fits the budget -- is copied and resident once.  A
// host stack of several chunks is copied a second time in pass 2 (the rows of the whole stack must be placed before a cloud can be
// written); the copy of chunk c + 1 does NOT overlap the scan of chunk c: the read-back of the meta words ends every chunk.
#include "nyxhip_ctx.h"
#include "volscan_plan.h"

using namespace nyxhip;

namespace {

bool dt_ok(int32_t dt) { return dt == NYXHIP_U8 || dt == NYXHIP_U16 || dt == NYXHIP_U32; }

size_t rows_bytes(uint64_t cap_rows) { return (size_t)kVsRowWords * vs_al256(4 * (size_t)cap_rows); }
void carve_rows(char* base, uint64_t cap_rows, VsRows& U)
{
    const size_t stride = vs_al256(4 * (size_t)cap_rows);
    uint32_t** const f[kVsRowWords] = {&U.vol, &U.label, &U.cnt, &U.x0, &U.y0, &U.z0, &U.w, &U.h, &U.d, &U.vmin, &U.vmax};
    for (int k = 0; k < kVsRowWords; k++) *f[k] = (uint32_t*)(base + (size_t)k * stride);
}

// the unsorted rows grown to `need` rows, the first `have` kept
int grow_unsorted(nyxhip_ctx* ctx, VsRows& U, uint64_t& cap_rows, uint64_t have, uint64_t need, hipStream_t st)
{
    VolScanBufs& S = ctx->volscan;
    if (need <= cap_rows && S.unsorted) return NYXHIP_OK;
    const uint64_t want = std::max<uint64_t>(need, 2 * cap_rows);
    if (have == 0) {
        HIP_TRY(ctx, S.unsorted.reserve(rows_bytes(want), st));
        cap_rows = want;
        carve_rows(S.unsorted.as<char>(), cap_rows, U);
        return NYXHIP_OK;
    }
    DevBuf nb;
    HIP_TRY(ctx, nb.reserve(rows_bytes(want), nullptr));
    VsRows N;
    carve_rows(nb.as<char>(), want, N);
    uint32_t* const src[kVsRowWords] = {U.vol, U.label, U.cnt, U.x0, U.y0, U.z0, U.w, U.h, U.d, U.vmin, U.vmax};
    uint32_t* const dst[kVsRowWords] = {N.vol, N.label, N.cnt, N.x0, N.y0, N.z0, N.w, N.h, N.d, N.vmin, N.vmax};
    for (int k = 0; k < kVsRowWords; k++) HIP_TRY(ctx, hipMemcpyAsync(dst[k], src[k], 4 * (size_t)have, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    S.unsorted = std::move(nb);
    cap_rows = want; U = N;
    return NYXHIP_OK;
}

struct Chunk { uint32_t v0, nv; uint64_t row0, rows; };

void forget_batch(VolScanBufs& S)
{
    memset(&S.batch, 0, sizeof(S.batch));
    S.batch.memory = NYXHIP_MEM_DEVICE;
    S.volume_index = nullptr;
    S.valid = false;
}

} // namespace

extern "C" {

int nyxhip_assemble_volumes(nyxhip_ctx* ctx, const nyxhip_volumes* v, nyxhip_batch3d* out_batch, const uint32_t** out_volume_index)
{
    if (ctx) forget_batch(ctx->volscan);                     // every call ends the batch of the one before, a refused call too
    if (!ctx || !v || !out_batch) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "assemble_volumes: null context / volumes / out_batch");
    if (!v->inten || !v->label) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "assemble_volumes: null inten / label");
    if (!dt_ok(v->inten_dtype) || !dt_ok(v->label_dtype))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "assemble_volumes: inten_dtype / label_dtype must be NYXHIP_U8, NYXHIP_U16 or NYXHIP_U32");
    if (v->memory != NYXHIP_MEM_HOST && v->memory != NYXHIP_MEM_DEVICE) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "assemble_volumes: bad volumes->memory");
    if (v->width == 0 || v->height == 0 || v->depth == 0 || v->n_volumes == 0)
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "assemble_volumes: width, height, depth and n_volumes must be non-zero");
    if (v->width > kVsMaxSide || v->height > kVsMaxSide || v->depth > kVsMaxSide)
        return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "assemble_volumes: a volume side exceeds " + std::to_string(kVsMaxSide) + " (coordinates inside an ROI are 16-bit)");
    const uint64_t vox = (uint64_t)v->width * v->height * v->depth;   // (each side < 2^16: no overflow)
    if (vox >= (1ull << 32)) return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "assemble_volumes: a volume of 2^32 voxels or more (voxel counts are 32-bit)");

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    VolScanBufs& S = ctx->volscan;
    hipStream_t st = ctx->stream();
    StreamDrain drain{st, st};                               // no copy out of the caller's volumes is in flight on any way out
    const bool host = v->memory == NYXHIP_MEM_HOST;
    const uint32_t nv = v->n_volumes;
    const int dti = v->inten_dtype, dtl = v->label_dtype;
    const uint64_t vol_bytes = vs_volume_bytes(vox, dti, dtl);

    size_t budget = (size_t)v->max_device_bytes;
    if (budget == 0) {
        size_t fr = 0, tot = 0;
        HIP_TRY(ctx, hipMemGetInfo(&fr, &tot));
        const int sharers = std::max(1, g_ctx_on_device[ctx->device & 63].load());
        budget = (fr + S.stage.bytes + S.table.bytes) / 2 / (size_t)sharers;
    }
    HIP_TRY(ctx, S.meta.reserve(4 * VS_META_WORDS, st));
    uint32_t* const meta = S.meta.as<uint32_t>();
    HIP_TRY(ctx, hipMemsetAsync(meta, 0, 4 * VS_META_WORDS, st));
    uint32_t h_meta[VS_META_WORDS];

    const uint32_t limit = vs_cap_limit(vox);
    uint32_t cap = vs_cap_first(limit, S.cap_hint);
    std::vector<Chunk> chunks;
    uint64_t n_rows = 0, cap_rows = 0;
    VsRows U = {};
    uint32_t staged_v0 = 0, staged_n = 0;                    // the volumes the staging buffer holds

    // volumes [c0, c0 + cn) in device memory: the caller's, or staged
    auto resident = [&](uint32_t c0, uint32_t cn, VsVolumes& V) -> int {
        V.dt_inten = dti; V.dt_label = dtl; V.W = v->width; V.H = v->height; V.D = v->depth; V.n = cn; V.v0 = c0;
        if (!host) {
            V.inten = (const char*)v->inten + (size_t)c0 * vox * dti;
            V.label = (const char*)v->label + (size_t)c0 * vox * dtl;
            return NYXHIP_OK;
        }
        const size_t o_lab = vs_al256((size_t)cn * vox * dti), total = o_lab + vs_al256((size_t)cn * vox * dtl);
        if (!(staged_n == cn && staged_v0 == c0)) {
            staged_n = 0;
            HIP_TRY(ctx, S.stage.reserve(total, st));
            HIP_TRY(ctx, staged_h2d(ctx, S.stage.p, (const char*)v->inten + (size_t)c0 * vox * dti, (size_t)cn * vox * dti, st));
            HIP_TRY(ctx, staged_h2d(ctx, S.stage.as<char>() + o_lab, (const char*)v->label + (size_t)c0 * vox * dtl, (size_t)cn * vox * dtl, st));
            staged_v0 = c0; staged_n = cn;
        }
        V.inten = S.stage.p; V.label = S.stage.as<char>() + o_lab;
        return NYXHIP_OK;
    };

    // ---- pass 1: scan, chunk by chunk ---------------------------------------------------------------------------------------
    for (uint32_t v0 = 0; v0 < nv;) {
        uint32_t nvc = vs_chunk_volumes(budget, host ? vol_bytes : 0, cap, nv - v0);
        // the slots and the z-planes of a chunk are counted in 32 bits
        nvc = (uint32_t)std::min<uint64_t>(nvc, std::max<uint64_t>(1, (1ull << 31) / cap));
        nvc = (uint32_t)std::min<uint64_t>(nvc, std::max<uint64_t>(1, 0xFFFFFFFFull / v->depth));
        if (nvc == 0)
            return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "assemble_volumes: one volume (" + std::to_string(host ? vol_bytes : 0) + " staged bytes) and its label table (" +
                                                           std::to_string(vs_table_bytes(cap)) + " bytes) do not fit max_device_bytes");
        VsVolumes V;
        if (int rc = resident(v0, nvc, V)) return rc;
        const uint64_t n_entries = (uint64_t)cap * nvc;
        const size_t o_blk = vs_al256(vs_table_bytes(cap) * nvc);
        HIP_TRY(ctx, S.table.reserve(o_blk + 4 * ((n_entries + kVsScanThreads - 1) / kVsScanThreads), st));
        VsTable T;
        uint32_t** const f[kVsTableWords] = {&T.key, &T.cnt, &T.vmin, &T.vmax, &T.xmin, &T.xmax, &T.ymin, &T.ymax, &T.zmin, &T.zmax};
        for (int k = 0; k < kVsTableWords; k++) *f[k] = S.table.as<uint32_t>() + (size_t)k * n_entries;
        T.cap = cap; T.probes = vs_probes(cap, limit);
        uint32_t* const blk_rows = (uint32_t*)(S.table.as<char>() + o_blk);
        HIP_TRY(ctx, hipMemsetAsync(meta, 0, 4 * 2, st));    // VS_META_STATUS, VS_META_ROWS
        if (int rc = launch_vs_scan(V, T, meta, st)) return fail(ctx, NYXHIP_ERR_HIP, std::string("volume scan kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
        if (int rc = launch_vs_count(T, n_entries, blk_rows, meta, st)) return fail(ctx, NYXHIP_ERR_HIP, std::string("volume count kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
        HIP_TRY(ctx, hipMemcpyAsync(h_meta, meta, 4 * 2, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (h_meta[VS_META_STATUS]) {                        // a table overflowed: larger tables, the same chunk again
            const uint32_t next = vs_cap_next(cap, limit);
            if (next == 0)
                return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "assemble_volumes: a volume holds more than " + std::to_string(kVsCapMax) + " labels");
            cap = next;
            continue;
        }
        const uint64_t rows = h_meta[VS_META_ROWS];
        if (rows) {
            if (int rc = grow_unsorted(ctx, U, cap_rows, n_rows, n_rows + rows, st)) return rc;
            if (int rc = launch_vs_compact(T, n_entries, blk_rows, U, n_rows, v0, meta, st))
                return fail(ctx, NYXHIP_ERR_HIP, std::string("volume compaction kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
        }
        chunks.push_back({v0, nvc, n_rows, rows});
        n_rows += rows;
        v0 += nvc;
    }
    S.cap_hint = cap;
    if (n_rows > 0x7FFFFFFFull) return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "assemble_volumes: more than 2^31 - 1 ROIs in one stack");
    S.batch.max_device_bytes = v->max_device_bytes;
    if (n_rows == 0) {                                       // a stack without any label
        HIP_TRY(ctx, hipStreamSynchronize(st));
        S.valid = true;
        *out_batch = S.batch;
        if (out_volume_index) *out_volume_index = nullptr;
        return NYXHIP_OK;
    }

    // ---- the rows of the stack in (volume, label) order, extrema, offsets -----------------------------------------------------
    const uint64_t n = n_rows;
    HIP_TRY(ctx, hipMemcpyAsync(h_meta, meta, 4 * VS_META_WORDS, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const uint32_t sort_blocks = vs_sort_blocks(n);
    const uint64_t off_blocks = (n + kVsScanThreads - 1) / kVsScanThreads;
    const size_t o_k0 = 0, o_k1 = vs_al256(o_k0 + 8 * n), o_i0 = vs_al256(o_k1 + 8 * n), o_i1 = vs_al256(o_i0 + 4 * n), o_hist = vs_al256(o_i1 + 4 * n),
                 o_ns = vs_al256(o_hist + 4 * 256 * (size_t)sort_blocks), o_bs = vs_al256(o_ns + 4 * n), o_sb = vs_al256(o_bs + 16 * off_blocks),
                 sort_total = vs_al256(o_sb + 8 * (n + 1));
    HIP_TRY(ctx, S.sort.reserve(sort_total, st));
    char* const sb = S.sort.as<char>();
    unsigned long long* keys[2] = {(unsigned long long*)(sb + o_k0), (unsigned long long*)(sb + o_k1)};
    uint32_t* idx[2] = {(uint32_t*)(sb + o_i0), (uint32_t*)(sb + o_i1)};
    uint32_t* const hist = (uint32_t*)(sb + o_hist);
    uint32_t* const n_slab = (uint32_t*)(sb + o_ns);
    unsigned long long* const blk_sums = (unsigned long long*)(sb + o_bs);
    unsigned long long* const slab_base = (unsigned long long*)(sb + o_sb);
    if (int rc = launch_vs_keys(U, n, keys[0], idx[0], st)) return fail(ctx, NYXHIP_ERR_HIP, std::string("volume key kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
    int cur = 0;
    const int lp = vs_label_passes(h_meta[VS_META_MAX_LABEL]), vp = vs_volume_passes(nv);
    for (int p = 0; p < lp + vp; p++) {
        const int shift = p < lp ? 8 * p : 32 + 8 * (p - lp);
        if (int rc = launch_vs_sort_pass(keys[cur], idx[cur], keys[cur ^ 1], idx[cur ^ 1], n, shift, hist, st))
            return fail(ctx, NYXHIP_ERR_HIP, std::string("volume row sort: launch failed: ") + hipGetErrorString((hipError_t)rc));
        cur ^= 1;
    }
    const size_t o_off = rows_bytes(n);
    HIP_TRY(ctx, S.rows.reserve(o_off + 8 * (n + 1), st));
    VsRows R;
    carve_rows(S.rows.as<char>(), n, R);
    unsigned long long* const px_offset = (unsigned long long*)(S.rows.as<char>() + o_off);
    if (int rc = launch_vs_gather(U, idx[cur], n, R, n_slab, meta, st)) return fail(ctx, NYXHIP_ERR_HIP, std::string("volume row kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
    if (int rc = launch_vs_offsets(R.cnt, n_slab, n, blk_sums, px_offset, slab_base, st))
        return fail(ctx, NYXHIP_ERR_HIP, std::string("volume offset kernels: launch failed: ") + hipGetErrorString((hipError_t)rc));
    unsigned long long n_px = 0, n_slabs = 0;
    HIP_TRY(ctx, hipMemcpyAsync(h_meta, meta, 4 * VS_META_WORDS, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&n_px, px_offset + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&n_slabs, slab_base + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (n_slabs > 0x7FFFFFFFull) return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "assemble_volumes: the boxes of the stack take more than 2^31 - 1 slabs of the cloud launch");

    // ---- pass 2: the clouds --------------------------------------------------------------------------------------------------
    const size_t o_y = vs_al256(2 * (size_t)n_px), o_z = 2 * o_y, o_v = 3 * o_y;
    HIP_TRY(ctx, S.cloud.reserve(o_v + 4 * (size_t)n_px, st));
    uint16_t* const cx = S.cloud.as<uint16_t>();
    uint16_t* const cy = (uint16_t*)(S.cloud.as<char>() + o_y);
    uint16_t* const cz = (uint16_t*)(S.cloud.as<char>() + o_z);
    uint32_t* const cv = (uint32_t*)(S.cloud.as<char>() + o_v);
    const bool counted = n_slabs > n;                        // some box takes the slab form
    uint32_t* slab_cnt = nullptr;
    if (counted) {
        HIP_TRY(ctx, S.table.reserve(4 * (size_t)n_slabs, st));
        slab_cnt = S.table.as<uint32_t>();
    }
    for (const Chunk& c : chunks) {
        if (c.rows == 0) continue;
        VsVolumes V;
        if (int rc = resident(c.v0, c.nv, V)) return rc;
        unsigned long long s0 = 0, s1 = n_slabs;
        if (chunks.size() > 1) {
            HIP_TRY(ctx, hipMemcpyAsync(&s0, slab_base + c.row0, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipMemcpyAsync(&s1, slab_base + c.row0 + c.rows, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
        }
        if (int rc = launch_vs_clouds(V, R, px_offset, slab_base, c.row0, c.row0 + c.rows, s0, s1, counted, slab_cnt, cx, cy, cz, cv, st))
            return fail(ctx, NYXHIP_ERR_HIP, std::string("volume cloud kernel: launch failed: ") + hipGetErrorString((hipError_t)rc));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));

    nyxhip_batch3d& B = S.batch;
    B.n_roi = n; B.roi_label = R.label; B.px_offset = (const uint64_t*)px_offset;
    B.x = cx; B.y = cy; B.z = cz; B.inten = cv;
    B.bbox_w = R.w; B.bbox_h = R.h; B.bbox_d = R.d; B.min_inten = R.vmin; B.max_inten = R.vmax;
    B.slide_min = nullptr; B.slide_max = nullptr;
    B.memory = NYXHIP_MEM_DEVICE;
    B.max_px = h_meta[VS_META_MAX_PX]; B.max_bbox_cells = h_meta[VS_META_MAX_CELLS]; B.max_inten_range = h_meta[VS_META_MAX_RANGE];
    B.max_device_bytes = v->max_device_bytes;
    S.volume_index = R.vol;
    S.valid = true;
    *out_batch = B;
    if (out_volume_index) *out_volume_index = S.volume_index;
    return NYXHIP_OK;
}

int nyxhip_assembled_rows(nyxhip_ctx* ctx, uint32_t* out_labels, uint32_t* out_volume_index, uint64_t max_rows)
{
    if (!ctx) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "assembled_rows: null context");
    VolScanBufs& S = ctx->volscan;
    if (!S.valid) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "assembled_rows: the context holds no assembled batch");
    const uint64_t n = S.batch.n_roi;
    if (max_rows < n) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "assembled_rows: max_rows is smaller than the " + std::to_string(n) + " rows of the batch");
    if (n == 0) return NYXHIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream();
    if (out_labels) HIP_TRY(ctx, hipMemcpyAsync(out_labels, S.batch.roi_label, 4 * n, hipMemcpyDeviceToHost, st));
    if (out_volume_index) HIP_TRY(ctx, hipMemcpyAsync(out_volume_index, S.volume_index, 4 * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return NYXHIP_OK;
}

int nyxhip_release_volumes(nyxhip_ctx* ctx)
{
    if (!ctx) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "release_volumes: null context");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream()));
    VolScanBufs& S = ctx->volscan;
    for (DevBuf* b : {&S.rows, &S.cloud, &S.table, &S.unsorted, &S.sort, &S.stage, &S.meta}) b->release();
    forget_batch(S);
    return NYXHIP_OK;
}

} // extern "C"
