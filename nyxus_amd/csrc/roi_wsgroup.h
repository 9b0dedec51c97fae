// roi_wsgroup.h -- host/device interface of the whole-slide group unit (roi_wsgroup.hip): the three classes of the reference's
// *WHOLESLIDE* group that the family entry refuses in whole-slide mode -- ContourFeature, Smoms2D / Imoms2D_feature and
// RadialDistributionFeature against the four-corner contour -- as dense sweeps over the slides in place.  The classes claim no
// family bit: their table belongs to nyxhip_wsgroup_slides (nyxhip_wsgroup.hip).  Band cut and record layout: wsgroup_plan.h.
#pragma once
#include <stdint.h>
#include "wsgroup_plan.h"

namespace nyxhip {

struct WsArgs {
    const void* img;            // n_slides images of w x h elements of dt (NYXHIP_U8 / U16 / U32) back to back
    int dt;
    uint32_t w, h, n_slides;
    uint32_t ws_mask;           // NYXHIP_WS_*
    const uint32_t* vmax;       // [n_slides] the slides' maxima (roi_slide.hip); read for NYXHIP_WS_CONTOUR only
    uint64_t* partials;         // [n_slides][ws_bands(w, h)][kWsWords]
    uint64_t* centre;           // [n_slides][kWsCentreWords]
    uint64_t* bins;             // [n_slides][kWsBinWords], zero before the launch
    uint32_t wedge_tab;         // radial_wedge_tab()
    double* out;                // row t at out + t * ld
    uint64_t ld;
    int32_t col_contour, col_smoms, col_imoms, col_radial;   // first column of each block in the row (blocks of unset bits: unused)
};

// Enqueues every launch the mask needs on `stream`: sweep (moments + radial pass A), close, radial pass B, radial tail.
// Returns a hipError_t as int.
int launch_wsgroup(const WsArgs& a, void* stream);

} // namespace nyxhip
