"""Feature codes of the 2-D morphology entries (nyxhip_morph_batch / _tiles): BasicMorphologyFeatures, ContourFeature,
ConvexHullFeature and ExtremaFeature of the reference (featureset.h:46-60, :71-82, :136-143).

The codes lie inside the shape block, where every bit of the C ABI's family mask is spoken for, so they have a mask space of their
own (_abi.MORPH_*) and a class of their own (nyxus_amd.NyxusMorphology).  `featureset.expand`, `featureset.FAMILY_OF`,
`featureset.GROUPS` and class `Nyxus` do not know them and keep refusing them."""
from __future__ import annotations

from typing import Dict, List, Tuple

from . import _abi, featureset

BASIC = ["AREA_PIXELS_COUNT", "AREA_UM2", "CENTROID_X", "CENTROID_Y", "WEIGHTED_CENTROID_Y", "WEIGHTED_CENTROID_X", "MASS_DISPLACEMENT",
         "COMPACTNESS", "BBOX_YMIN", "BBOX_XMIN", "BBOX_HEIGHT", "BBOX_WIDTH", "DIAMETER_EQUAL_AREA", "EXTENT", "ASPECT_RATIO"]
CONTOUR = ["PERIMETER", "DIAMETER_EQUAL_PERIMETER", "EDGE_MEAN_INTENSITY", "EDGE_STDDEV_INTENSITY", "EDGE_MAX_INTENSITY", "EDGE_MIN_INTENSITY",
           "EDGE_INTEGRATED_INTENSITY"]
HULL = ["CIRCULARITY", "CONVEX_HULL_AREA", "SOLIDITY"]          # CIRCULARITY is written by ConvexHullFeature from PERIMETER
EXTREMA = ["EXTREMA_P%d_%s" % (k, a) for k in range(1, 9) for a in "XY"]
ALL_MORPH = BASIC + CONTOUR + HULL + EXTREMA                     # the column order of _abi.MORPH_ALL

MORPH_OF: Dict[str, int] = {}
for _codes, _bit in ((BASIC, _abi.MORPH_BASIC), (CONTOUR, _abi.MORPH_CONTOUR), (HULL, _abi.MORPH_HULL), (EXTREMA, _abi.MORPH_EXTREMA)):
    for _n in _codes:
        MORPH_OF[_n] = _bit

# the group token the entries serve completely (featureset.cpp: FG2_BASIC_MORPHOLOGY)
GROUPS_MORPH: Dict[str, List[str]] = {"*BASIC_MORPHOLOGY*": BASIC}
# *ALL_MORPHOLOGY* (convex_hull.h:12-20 and the group table) also enables these three, which are a closing formula over NUM_NEIGHBORS,
# PERIMETER, CONVEX_HULL_AREA and the Feret diameters and are not served
ALL_MORPHOLOGY_MISSING = ["POLYGONALITY_AVE", "HEXAGONALITY_AVE", "HEXAGONALITY_STDDEV"]

# featureset.IH_REQUEST_ORDER with the 41 codes at their enum positions: BASIC in front of MAJOR_AXIS_LENGTH, the contour and hull codes
# between ROUNDNESS and EROSIONS_2_VANISH, the extrema between EULER_NUMBER and DIAMETER_MIN_ENCLOSING_CIRCLE
_O = featureset.IH_REQUEST_ORDER
_A, _B, _C = _O.index("MAJOR_AXIS_LENGTH"), _O.index("ROUNDNESS") + 1, _O.index("EULER_NUMBER") + 1
assert _O[_B] == "EROSIONS_2_VANISH" and _O[_C] == "DIAMETER_MIN_ENCLOSING_CIRCLE"
MORPH_REQUEST_ORDER: List[str] = _O[:_A] + BASIC + _O[_A:_B] + CONTOUR + HULL + _O[_B:_C] + EXTREMA + _O[_C:]


def expand_morph(features: List[str]) -> Tuple[int, int, List[str]]:
    """(the family mask as featureset.expand gives it -- 0 when every requested code is a morphology code --, the morphology mask, the
    requested codes in enum order).  Everything this module does not own goes through featureset.expand, errors included."""
    mine, rest = set(), []
    for f in features:
        key = f.strip().upper()
        if key == "*ALL_MORPHOLOGY*":
            raise ValueError(f"the group *ALL_MORPHOLOGY* is not served by the MI355X path: it also enables {', '.join(ALL_MORPHOLOGY_MISSING)} "
                             "(a closing formula over the neighbor count, the perimeter, the hull area and the Feret diameters), which are not "
                             "served.  Request *BASIC_MORPHOLOGY* and the individual codes instead")
        if key in GROUPS_MORPH:
            mine.update(GROUPS_MORPH[key])
        elif key in MORPH_OF:
            mine.add(key)
        else:
            rest.append(f)
    fam_mask, fam_codes = featureset.expand(rest) if rest else (0, [])
    if not mine and not fam_codes:
        raise ValueError("no features requested")
    want = mine | set(fam_codes)
    ordered = [n for n in MORPH_REQUEST_ORDER if n in want]
    mmask = 0
    for n in mine:
        mmask |= MORPH_OF[n]
    return fam_mask, mmask, ordered
