// vol_plan.h -- the arithmetic of the volume entries' workspaces, in plain C++ (no HIP: tests/cpp/test_vol_plan.cpp includes it with g++):
// the ROIs of a chunk, the largest box sides of a batch, and per entry the strides of its *Args and the workspace bytes of one ROI.
// The entries (nyxhip_vol*.hip) carve their workspace by these strides; vol_host.h has what needs the device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/nyxhip.h"
#include "roi_vol.h"
#include "roi_voltex.h"
#include "roi_volzone.h"
#include "roi_voldzone.h"
#include "roi_volshape.h"

namespace nyxhip {

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// ROIs per chunk of a batch of n_roi >= 1 whose ROIs take per_roi workspace bytes each: min(budget / per_roi, 65535, n_roi) (a grid
// dimension counts the ROIs of a chunk); 0: one ROI does not fit the budget.  per_roi == 0: no workspace, the budget is not read.
inline uint64_t vol_chunk(size_t per_roi, size_t budget, uint64_t n_roi)
{
    const uint64_t most = n_roi < 65535 ? n_roi : 65535;
    if (per_roi == 0) return most;
    const uint64_t fit = budget / per_roi;
    return fit < most ? fit : most;
}

// The largest box sides of a batch and its largest vdz_pitch(w, h), over the ROIs the device admits: sides up to kVolMaxSide and at
// most max_cells cells (the others are refused on the device and size nothing).  No admitted ROI: sides 1, the pitch of a 1 x 1 box.
struct VolSides { uint32_t side_max[3]; uint32_t pitch_max; };
inline VolSides vol_sides(uint64_t nr, const uint32_t* bw, const uint32_t* bh, const uint32_t* bd, uint32_t max_cells)
{
    VolSides m = {{1u, 1u, 1u}, vdz_pitch(1u, 1u)};
    for (uint64_t r = 0; r < nr; r++) {
        const uint32_t w = bw[r], h = bh[r], d = bd[r];
        if (w > kVolMaxSide || h > kVolMaxSide || d > kVolMaxSide || (uint64_t)w * h * d > (uint64_t)max_cells) continue;
        if (w > m.side_max[0]) m.side_max[0] = w;
        if (h > m.side_max[1]) m.side_max[1] = h;
        if (d > m.side_max[2]) m.side_max[2] = d;
        if (vdz_pitch(w, h) > m.pitch_max) m.pitch_max = vdz_pitch(w, h);
    }
    return m;
}

// Each *_layout below writes into `a` what the strides rest on (the greyInfo of the classes, the extrema) and the strides, and returns
// the workspace bytes of one ROI.  The order of the regions inside the workspace is the entry's own.

// nyxhip_featurize_volumes: a binned box for the GLCM block, two sort buffers of keys for the intensity block
inline size_t vol_layout(VolArgs& a, uint32_t vmask, const nyxhip_settings* s, uint32_t max_px, uint32_t max_cells)
{
    a.grey_info = s->ibsi ? 0 : s->glcm_grey_depth;       // 3d_glcm.cpp:51-53
    a.max_cells = max_cells ? max_cells : 1u; a.max_px = max_px ? max_px : 1u;
    a.box_stride = (vmask & NYXHIP_VFAM_GLCM) ? al256(a.max_cells) : 0;
    a.key_stride = (vmask & NYXHIP_VFAM_INTENSITY) ? (al256(4 * (size_t)a.max_px) >> 2) : 0;
    return a.box_stride + 8 * (size_t)a.key_stride;
}

// nyxhip_featurize_volumes_tex: a table per class and a binned box per class; GLDM and NGTDM share a box when they share a greyInfo,
// NGTDM at radius 0 needs neither a box nor a table
struct VoltexLayout { size_t per_roi, tab_words; bool tsweep, share; };
inline VoltexLayout voltex_layout(VoltexArgs& a, uint32_t tmask, const nyxhip_settings* s, const nyxhip_voltex_settings* t, uint32_t max_cells)
{
    const bool gldm = (tmask & NYXHIP_VTEX_GLDM) != 0, ngldm = (tmask & NYXHIP_VTEX_NGLDM) != 0, ngtdm = (tmask & NYXHIP_VTEX_NGTDM) != 0;
    a.g_gldm = s->ibsi ? 0 : t->gldm_grey_depth;           // 3d_gldm.cpp:93-95
    a.g_ngtdm = s->ibsi ? 0 : t->ngtdm_grey_depth;         // 3d_ngtdm.cpp:195-197
    a.radius = t->ngtdm_radius;
    a.max_cells = max_cells ? max_cells : 1u;
    a.box_stride = al256(a.max_cells);
    VoltexLayout L;
    L.tsweep = ngtdm && a.radius > 0;
    L.share = gldm && L.tsweep && a.g_gldm == a.g_ngtdm;
    const int nbox = (gldm ? 1 : 0) + (ngldm ? 1 : 0) + (L.tsweep && !L.share ? 1 : 0);
    a.tab_stride[VT_GLDM] = gldm ? al256(4 * (size_t)kVtGldmWords) >> 2 : 0;
    a.tab_stride[VT_NGLDM] = ngldm ? al256(4 * (size_t)kVtNgldmWords) >> 2 : 0;
    a.tab_stride[VT_NGTDM] = L.tsweep ? al256(4 * (size_t)vt_ngtdm_words(a.radius)) >> 2 : 0;
    L.tab_words = a.tab_stride[0] + a.tab_stride[1] + a.tab_stride[2];
    L.per_roi = (size_t)nbox * a.box_stride + 4 * L.tab_words;
    return L;
}

// nyxhip_featurize_volumes_zones: the run tables sized by the largest box sides, the zone tables, labels, counts and keys, and a binned
// box per class; the classes share a box when they share a greyInfo
struct VolzoneLayout { size_t per_roi, tab_words; bool share; };
inline VolzoneLayout volzone_layout(VolzoneArgs& a, uint32_t zmask, const nyxhip_settings* s, const nyxhip_volzone_settings* t, uint32_t max_cells,
                                    const VolSides& sides)
{
    const bool rl = (zmask & NYXHIP_VZONE_GLRLM) != 0, sz = (zmask & NYXHIP_VZONE_GLSZM) != 0;
    a.g[VZ_GLRLM] = s->ibsi ? 0 : t->glrlm_grey_depth;     // 3d_glrlm.cpp:147-149
    a.g[VZ_GLSZM] = s->ibsi ? 0 : t->glszm_grey_depth;     // 3d_glszm.cpp:490-492
    for (int c = 0; c < 2; c++) a.rows[c] = (a.g[c] ? (uint32_t)abs(a.g[c]) : kVzLevelCap) + 1u;
    a.max_cells = max_cells ? max_cells : 1u;
    a.box_stride = al256(a.max_cells);
    for (int ax = 0; ax < 3; ax++) a.side_max[ax] = sides.side_max[ax];
    VolzoneLayout L;
    L.share = rl && sz && a.g[VZ_GLRLM] == a.g[VZ_GLSZM];
    const int nbox = (rl ? 1 : 0) + (sz ? 1 : 0) - (L.share ? 1 : 0);
    if (rl) {
        size_t rl_words = kVzRlHead;
        for (int k = 0; k < kVzDirs; k++) {
            a.rl_dir_off[k] = rl_words;
            rl_words += (size_t)a.rows[VZ_GLRLM] * vz_dir_len(kVzShifts[k][0], kVzShifts[k][1], kVzShifts[k][2], a.side_max[0], a.side_max[1], a.side_max[2]);
        }
        a.rl_stride = al256(4 * rl_words) >> 2;
    }
    if (sz) {
        a.sz_stride = al256(4 * (size_t)(kVzSzHead + a.rows[VZ_GLSZM] * kVzDenseSizes)) >> 2;
        a.cell_stride = al256(4 * (size_t)a.max_cells) >> 2;
        a.key_stride = al256(4 * ((size_t)a.max_cells / (kVzDenseSizes + 1u) + 1u)) >> 2;
    }
    L.tab_words = a.rl_stride + a.sz_stride;
    L.per_roi = (size_t)nbox * a.box_stride + 4 * (L.tab_words + 2 * a.cell_stride + 2 * a.key_stride);
    return L;
}

// nyxhip_featurize_volumes_dzones: the table sized by the largest min(w, h) of the batch, labels, minima, distances and one binned box
inline size_t voldzone_layout(VoldzoneArgs& a, const nyxhip_settings* s, uint32_t max_cells, const VolSides& sides)
{
    a.g = s->ibsi ? 0 : s->grey_depth;                     // 3d_gldzm.cpp:68-73: n_levels is never set
    a.rows = (a.g ? (uint32_t)abs(a.g) : kVzLevelCap) + 1u;
    a.max_cells = max_cells ? max_cells : 1u;
    a.box_stride = al256(a.max_cells);
    for (int ax = 0; ax < 3; ax++) a.side_max[ax] = sides.side_max[ax];
    a.pitch_max = sides.pitch_max;
    a.tab_stride = al256(4 * ((size_t)kVdzHead + (size_t)a.rows * a.pitch_max)) >> 2;
    a.cell_stride = al256(4 * (size_t)a.max_cells) >> 2;
    a.dist_stride = al256(2 * (size_t)a.max_cells) >> 1;
    return a.box_stride + 4 * a.tab_stride + 2 * a.dist_stride + 8 * a.cell_stride;
}

// nyxhip_featurize_volumes_shape: the head, the row extremes and the occupancy box (zeroed per chunk), then the chains, the candidates,
// the visited set and the edge stack of the hull, all sized by the (z, y) rows of the largest box sides of the batch
struct VolshapeLayout { size_t per_roi, zeroed; };
inline VolshapeLayout volshape_layout(VolshapeArgs& a, uint32_t max_px, uint32_t max_cells, const VolSides& sides)
{
    a.max_cells = max_cells ? max_cells : 1u; a.max_px = max_px ? max_px : 1u;
    for (int ax = 0; ax < 3; ax++) a.side_max[ax] = sides.side_max[ax];
    const uint64_t rows = (uint64_t)a.side_max[1] * a.side_max[2];
    a.rows_max = (uint32_t)(rows < a.max_cells ? rows : a.max_cells);
    a.row_stride = al256(4 * (size_t)a.rows_max) >> 2;
    a.occ_stride = al256(a.max_cells);
    a.cand_stride = 2 * a.row_stride;
    a.lds_cand = (uint32_t)(a.cand_stride < kVshLdsCand ? a.cand_stride : kVshLdsCand);
    a.visited_stride = vsh_table(a.cand_stride);
    a.stack_stride = 3 * a.cand_stride;
    VolshapeLayout L;
    L.zeroed = 8 * (size_t)kVshHead + 8 * a.row_stride + a.occ_stride;
    L.per_roi = L.zeroed + 8 * a.row_stride + 8 * (a.cand_stride + a.visited_stride + a.stack_stride);
    return L;
}

} // namespace nyxhip
