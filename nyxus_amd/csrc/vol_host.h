// vol_host.h -- host code the two volume entry files share (nyxhip_vol.hip defines it, nyxhip_voltex.hip uses it).
#pragma once
#include <functional>
#include "nyxhip_ctx.h"

namespace nyxhip {

// the device batch of the call (a host batch: staged), the device table and its leading dimension, the extrema the strides are sized by
using VolBody = std::function<int(const nyxhip_batch3d& dev, double* d_out, size_t ld, uint32_t max_px, uint32_t max_cells)>;

int vol_run(nyxhip_ctx* ctx, const nyxhip_batch3d* b, bool glcm, size_t ncol, double* out, size_t ld, const VolBody& body, int (*check)(nyxhip_ctx*));
// the workspace budget of a call: max_device_bytes, or half of the free device memory (`held`: what the workspace buffer already holds)
int vol_budget(nyxhip_ctx* ctx, const nyxhip_batch3d* b, size_t held, size_t& budget);
int vol_scan(nyxhip_ctx* ctx, uint64_t nr, const uint64_t* off, const uint32_t* w, const uint32_t* h, const uint32_t* d, uint32_t& max_px, uint32_t& max_cells);

} // namespace nyxhip
