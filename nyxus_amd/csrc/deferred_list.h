// deferred_list.h -- the ROIs a family's LDS launch leaves out, served afterwards from a global workspace (internal).
// A launch carves its LDS for a cap; a classifier appends the index of every ROI beyond the cap to a list, the host reads the count
// back, sizes a per-workgroup workspace and launches the family's kernel over the list, in chunks when the workspace budget says so.
//   device buffer: [0 .. 64) header: [0] ROIs listed, [1 .. 3] maxima a predicate records with atomicMax | [64 .. 64 + n_roi) the list
//   chunk launch:  workgroup b serves ROI list[o + b] from workspace slot b (the kernels index their workspace by blockIdx.x)
// Three parts: the chunk arithmetic (plain C++) | in a kernel unit: the classifier, instantiated there for the predicate the unit owns
// (no device code crosses a unit) | in a host unit (behind nyxhip_ctx.h): the steps build / count / chunks.
#pragma once
#include <stdint.h>
#include "knobs.h"

namespace nyxhip {

// ROIs per chunk launch of n listed ROIs: max(1, min(n, budget / stride)); 0: the stride is zero (deferred_chunks reports it).
inline uint64_t deferred_chunk(uint64_t n, uint64_t stride_bytes, uint64_t budget_bytes)
{
    if (stride_bytes == 0) return 0;
    const uint64_t fit = budget_bytes / stride_bytes, most = fit < n ? fit : n;
    return most < 1 ? 1 : most;
}

constexpr uint32_t kDeferredHdrWords = 64;

#ifdef __HIPCC__
// Enqueues the classifier of `Pred` over ROIs 0 .. n_roi on `st`; 0 or the hipError_t.  pred(i, hdr): is ROI i listed?
template <class Pred> int deferred_classify(uint64_t n_roi, const Pred& pred, uint32_t* hdr, hipStream_t st);

// predicate of the contour chain's list (roi_moments.hip): ROIs whose padded flag plane, (w + 2)(h + 2) bytes, exceeds `cap`
struct ContourPlaneBig { const uint32_t *bw, *bh; uint32_t cap; __device__ bool operator()(uint64_t i, uint32_t* hdr) const; };

#ifndef HIP_TRY   // a kernel unit
template <class Pred> __global__ void deferred_classify_kernel(uint64_t n_roi, const Pred pred, uint32_t* hdr)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < n_roi && pred(i, hdr))
        hdr[kDeferredHdrWords + atomicAdd(&hdr[0], 1u)] = (uint32_t)i;
}

template <class Pred> int deferred_classify(uint64_t n_roi, const Pred& pred, uint32_t* hdr, hipStream_t st)
{
    if (n_roi == 0) return 0;
    hipLaunchKernelGGL(deferred_classify_kernel<Pred>, dim3((unsigned)((n_roi + 255) / 256)), dim3(256), 0, st, n_roi, pred, hdr);
    return (int)hipGetLastError();
}
#else             // a host unit
struct DeferredList {
    uint32_t* d_hdr = nullptr;         // the device buffer
    uint32_t hdr[4] = {};              // header words [0 .. 3] on the host, once deferred_count has run
    const uint32_t* list() const { return d_hdr + kDeferredHdrWords; }
};

// build: list buffer, cleared header, classifier -- all on `st`, nothing waited for
template <class Pred>
int deferred_build(nyxhip_ctx* ctx, const char* site, DevBuf& buf, uint64_t n_roi, const Pred& pred, hipStream_t st, DeferredList& dl)
{
    HIP_TRY(ctx, buf.reserve(4 * kDeferredHdrWords + 4 * (size_t)n_roi, st));
    dl.d_hdr = buf.as<uint32_t>();
    HIP_TRY(ctx, hipMemsetAsync(dl.d_hdr, 0, 4 * kDeferredHdrWords, st));
    return deferred_classify(n_roi, pred, dl.d_hdr, st) != 0 ? fail(ctx, NYXHIP_ERR_HIP, std::string(site) + " classifier: launch failed") : NYXHIP_OK;
}

// count: header words [0 .. 3] to the host; the site's one synchronisation of `st`
inline int deferred_count(nyxhip_ctx* ctx, DeferredList& dl, hipStream_t st)
{
    HIP_TRY(ctx, hipMemcpyAsync(dl.hdr, dl.d_hdr, sizeof(dl.hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return NYXHIP_OK;
}

// chunks: `ws` grows to chunk * stride_bytes, then launch(list + o, count) -> NYXHIP_OK or the site's error, chunk after chunk
template <class Launch>
int deferred_chunks(nyxhip_ctx* ctx, const char* site, const DeferredList& dl, uint64_t stride_bytes, size_t budget, DevBuf& ws, hipStream_t st,
                    Launch&& launch)
{
    const uint64_t n = dl.hdr[0], chunk = deferred_chunk(n, stride_bytes, knob::large_budget(budget));
    if (chunk == 0) return fail(ctx, NYXHIP_ERR_HIP, std::string(site) + ": listed ROIs with an empty workspace");
    HIP_TRY(ctx, ws.reserve((size_t)(stride_bytes * chunk), st));
    for (uint64_t o = 0; o < n; o += chunk)
        if (int rc = launch(dl.list() + o, (uint32_t)(n - o < chunk ? n - o : chunk))) return rc;
    return NYXHIP_OK;
}
#endif
#endif

} // namespace nyxhip
