"""nyxus_amd.NyxusWholeSlide -- class `NyxusAllMorphology` plus the group *WHOLESLIDE* and, in whole-slide mode (single_roi=True, or a
directory without label images), the three classes of that group the older classes refuse there: the contour codes, the two moment
classes and the radial distribution, served by nyxhip_wsgroup_slides against the slide's four-corner contour.

The group is the reference's FG2_WHOLESLIDE (env_features.cpp:219-234): the codes of ContourFeature, PixelIntensityFeatures, GLCM, GLDM,
GLRLM, GLSZM, NGLDM, NGTDM, Gabor, Imoms2D_feature, RadialDistributionFeature and Zernike, in enum order.  GLDZM and the shape moments
are not in it.  With label images it is a plain expansion over entries that already exist.  `Nyxus`, `NyxusMorphology` and
`NyxusAllMorphology` keep raising on the group, and in whole-slide mode on the codes.

In whole-slide mode the codes of family bits 0-9 go through nyxhip_featurize_slides as in `Nyxus`; the contour, *SGEOMOMS* / *IGEOMOMS*
and radial codes go through nyxhip_wsgroup_slides; the tables are joined and the columns selected by name in enum order.  Every other
code (hull, basic morphology, extrema, neighbors, intensity histogram, the other shape families) is refused by name before a context
exists.

ONE QUIRK OF THE REFERENCE IS KEPT.  It builds the four-corner contour in this mode only when a contour-dependent class is requested
(reduce_trivial_rois.cpp:446-457); the moment classes count as such, RadialDistributionFeature itself does not.  FRAC_AT_D, MEAN_FRAC and
RADIAL_CV requested without any contour or moment code are therefore 24 zeros in the reference, and here: the class returns those zeros
without a device call for the radial block.  With *WHOLESLIDE* the contour exists."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List

import numpy as np

from . import _abi, _lib, featureset, featureset_allmorph, featureset_morph
from .nyxus_allmorph import NyxusAllMorphology

# the `featureset` member of every class FG2_WHOLESLIDE enables, in the order of env_features.cpp:221-232
WHOLESLIDE_CLASSES: Dict[str, List[str]] = {
    "ContourFeature": featureset_morph.CONTOUR,
    "PixelIntensityFeatures": featureset.INTENSITY,
    "GLCMFeature": featureset.GLCM_ANGLED + featureset.GLCM_AVE,
    "GLDMFeature": featureset.GLDM,
    "GLRLMFeature": featureset.GLRLM_ANGLED + featureset.GLRLM_AVE,
    "GLSZMFeature": featureset.GLSZM,
    "NGLDMfeature": featureset.NGLDM,
    "NGTDMFeature": featureset.NGTDM,
    "GaborFeature": ["GABOR"],
    "Imoms2D_feature": featureset.IMOMS,
    "RadialDistributionFeature": featureset.RADIAL,
    "ZernikeFeature": ["ZERNIKE2D"],
}
_IN_GROUP = {c for codes in WHOLESLIDE_CLASSES.values() for c in codes}
WHOLESLIDE: List[str] = [c for c in featureset_allmorph.ALL_MORPH_REQUEST_ORDER if c in _IN_GROUP]      # enum order
assert len(WHOLESLIDE) == len(_IN_GROUP)
GROUPS_WHOLESLIDE: Dict[str, List[str]] = {"*WHOLESLIDE*": WHOLESLIDE}

# whole-slide mode: the codes nyxhip_wsgroup_slides serves, by bit of its mask
WS_OF: Dict[str, int] = {}
for _codes, _bit in ((featureset_morph.CONTOUR, _abi.WS_CONTOUR), (featureset.SMOMS, _abi.WS_SMOMS), (featureset.IMOMS, _abi.WS_IMOMS),
                     (featureset.RADIAL, _abi.WS_RADIAL)):
    for _n in _codes:
        WS_OF[_n] = _bit
_NEEDS_CONTOUR = _abi.WS_CONTOUR | _abi.WS_SMOMS | _abi.WS_IMOMS       # the classes that make the reference build the contour


def expand_wholeslide(features: List[str]) -> List[str]:
    """`features` with the group token replaced by its codes; everything else untouched (the classes below validate it)."""
    out: List[str] = []
    for f in features:
        out += GROUPS_WHOLESLIDE.get(f.strip().upper(), [f])
    return out


class NyxusWholeSlide(NyxusAllMorphology):
    def _set_features(self, features: List[str]):
        super()._set_features(expand_wholeslide(list(features)))
        self._features = list(features)

    def _ws_masks(self):
        """(the mask of nyxhip_wsgroup_slides, whether the radial codes are the reference's 24 zeros) of the request."""
        want = 0
        for c in self._requested:
            want |= WS_OF.get(c, 0)
        radial_zeros = bool(want & _abi.WS_RADIAL) and not (want & _NEEDS_CONTOUR)
        return (want & ~_abi.WS_RADIAL if radial_zeros else want), radial_zeros

    def _whole_slide_refusals(self):
        """Whole-slide mode serves the families of bits 0-9 and the codes of WS_OF; every other requested code is an error raised
        before anything touches the device."""
        bad = [c for c in self._requested if c not in WS_OF and (c not in featureset.FAMILY_OF or featureset.FAMILY_OF[c] & ~_abi.FAM_WHOLE_SLIDE)]
        if bad:
            raise ValueError(f"feature(s) {bad} are not served in whole-slide mode (single_roi=True, or a directory without label images): "
                             "it serves the *WHOLESLIDE* group, the GLDZM family and the shape moments")

    def _featurize_slides(self, intensity_files: list):
        """As Nyxus._featurize_slides, with the table of nyxhip_wsgroup_slides to the right of the family table."""
        import pandas as pd
        from . import tiff_ingest
        self._whole_slide_refusals()
        requested, _ = self._active()
        fam = self._mask & _abi.FAM_WHOLE_SLIDE
        ws, radial_zeros = self._ws_masks()
        names = _lib.column_names(fam, self._settings) if fam else []
        if ws:
            names = names + _lib.wsgroup_column_names(ws)
        if radial_zeros:
            names = names + _lib.wsgroup_column_names(_abi.WS_RADIAL)
        angles = [self._settings.glcm_angles[i] for i in range(self._settings.glcm_n_angles)]
        sel = featureset.column_selector(requested, names, angles)
        cols = [names[i] for i in sel]
        blocks = []

        def flush(stack):
            if not stack:
                return
            S = np.stack(stack)
            parts = []
            if fam:
                parts.append(self._context().featurize_slides_host(S, fam, self._settings, max_device_bytes=self._device_budget()))
            if ws:
                parts.append(self._context().wsgroup_slides_host(S, ws, self._settings, max_device_bytes=self._device_budget()))
            if radial_zeros:
                parts.append(np.zeros((len(stack), _abi.WS_COLS[_abi.WS_RADIAL])))
            table = np.ascontiguousarray(np.hstack(parts))
            _lib.load().nyxhip_finalize_table(table.ctypes.data, table.shape[0], table.shape[1], table.shape[1], C.c_double(self._settings.soft_nan))
            blocks.append(table[:, sel])

        stack = []
        for f in intensity_files:
            I = tiff_ingest.read_tiff(f)
            if I.dtype not in (np.uint8, np.uint16, np.uint32):
                I = I.astype(np.uint32)
            if stack and (I.shape != stack[0].shape or I.dtype != stack[0].dtype or len(stack) * I.nbytes > (1 << 30)):
                flush(stack)
                stack = []
            stack.append(I)
        flush(stack)
        n = len(intensity_files)
        df = pd.DataFrame(np.concatenate(blocks) if blocks else np.zeros((0, len(cols))), columns=cols)
        df.insert(0, "t_index", np.zeros(n))
        df.insert(0, "ROI_label", np.ones(n, np.uint32))
        df.insert(0, "mask_image", np.asarray([""] * n, dtype=object))
        df.insert(0, "intensity_image", np.asarray([str(f) for f in intensity_files], dtype=object))
        return df
