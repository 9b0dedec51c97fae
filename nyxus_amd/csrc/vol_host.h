// vol_host.h -- the host path the four volume entry files share (nyxhip_vol.hip defines it; nyxhip_voltex.hip, nyxhip_volzone.hip and
// nyxhip_voldzone.hip use it): the checks every entry starts with, the extrema, the staging of a host batch, the box sides of the batch,
// the chunks of ROIs under the device budget, the binned boxes, the texts of the device status.  What an entry file keeps is its own:
// its catalogue, its cap checks, the filling of its *Args, the order of the regions in its workspace and its launches per chunk.  The
// arithmetic that needs no device is in vol_plan.h.
#pragma once
#include <functional>
#include "nyxhip_ctx.h"
#include "vol_plan.h"

namespace nyxhip {

// what an entry's messages are made of
struct VolTexts {
    const char* label;         // the family, ahead of every message of the device status and of the chunk planner
    const char* settings;      // the settings pointers of the entry, as the first check names them
    const char* arrays;        // the arrays of the batch the entry reads, as the null-pointer check names them
    std::string cap;           // the level cap, as the entry's refusals state it
    const char* unbinned;      // NYXHIP_ERR_UNSUPPORTED on the device: when the levels are the intensities
    const char* outside;       // NYXHIP_ERR_INVALID_ARG on the device: what else than a voxel outside its box raises it ("": nothing)
    const char* internal;      // NYXHIP_ERR_INTERNAL on the device; NULL: the entry's kernels never raise it
    bool sides;                // the entry sizes its workspace by the box sides of the batch (VolSides)
};
// (x, y, z and the boxes are read by every entry but the intensity block of nyxhip_featurize_volumes alone)
constexpr const char* kVolArraysAll = "(px_offset, x, y, z, inten, bbox_w, bbox_h, bbox_d, min_inten, max_inten)";

// The checks every entry starts with, in the order they fire: null batch / settings / table, the mask (`bad_mask`: NULL or the text of
// its refusal), null arrays (`boxes`: the entry reads coordinates and boxes), slide_min without slide_max (`slide_pair`: the entry reads
// them), out_ld, the ROI count, batch->memory.
int vol_entry_checks(nyxhip_ctx* ctx, const VolTexts& tx, const nyxhip_batch3d* b, bool have_settings, const double* out, const char* bad_mask, bool boxes,
                     bool slide_pair, size_t ncol, size_t ld);

// the device batch of the call (a host batch: staged), the device table and its leading dimension, the extrema the strides are sized by,
// the box sides of the batch (VolTexts::sides; otherwise all 1)
using VolBody = std::function<int(const nyxhip_batch3d& dev, double* d_out, size_t ld, uint32_t max_px, uint32_t max_cells, const VolSides& sides)>;

int vol_run(nyxhip_ctx* ctx, const VolTexts& tx, const nyxhip_batch3d* b, bool boxes, size_t ncol, double* out, size_t ld, const VolBody& body);
int vol_scan(nyxhip_ctx* ctx, uint64_t nr, const uint64_t* off, const uint32_t* w, const uint32_t* h, const uint32_t* d, uint32_t& max_px, uint32_t& max_cells);
// The ROIs per chunk of a call whose ROIs take per_roi workspace bytes each, and ctx->d_vol grown to a chunk of them.  The budget is
// max_device_bytes, or half of the free device memory; per_roi == 0: no budget is read and nothing reserved.
int vol_plan_chunks(nyxhip_ctx* ctx, const VolTexts& tx, const nyxhip_batch3d& b, size_t per_roi, uint64_t& chunk);
// The binned boxes of the chunk [roi0, roi0 + n_roi) (vol_bin_kernel: bin_intensities_3d with the class's greyInfo): the cells outside
// the cloud hold the background level.  vol_bin_launch: for a VolArgs that is filled already.
int vol_bin(nyxhip_ctx* ctx, const nyxhip_batch3d& b, uint64_t roi0, uint64_t n_roi, unsigned char* boxes, uint64_t box_stride, int grey_info, uint32_t max_px,
            uint32_t max_cells);
int vol_bin_launch(nyxhip_ctx* ctx, const VolArgs& v);
// a launch_* return code -> NYXHIP_OK, or NYXHIP_ERR_HIP with "<what>: launch failed: <the HIP error>"
int launched(nyxhip_ctx* ctx, int rc, const char* what);

} // namespace nyxhip
