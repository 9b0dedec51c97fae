"""Feature codes of the hexagonality / polygonality entries (nyxhip_hexpoly_batch / _tiles) and the group *ALL_MORPHOLOGY*.

HexagonalityPolygonalityFeature (featureset.h:146-148 of the reference) closes ConvexHullFeature::featureset (convex_hull.h:12-20),
the last of the sixteen classes the group enables (env_features.cpp:254-274) that the path did not serve completely.  The codes follow
the subclass convention of `featureset_morph`: `featureset.expand`, `featureset_morph.expand_morph`, class `Nyxus` and class
`NyxusMorphology` do not know them and keep refusing them; `expand_all_morph` and class `nyxus_amd.NyxusAllMorphology` serve them."""
from __future__ import annotations

from typing import Dict, List, Tuple

from . import featureset, featureset_morph

HEXPOLY = ["POLYGONALITY_AVE", "HEXAGONALITY_AVE", "HEXAGONALITY_STDDEV"]
assert HEXPOLY == featureset_morph.ALL_MORPHOLOGY_MISSING

# the `featureset` member of every class FG2_MORPHOLOGY enables, in the order of env_features.cpp:256-271
ALL_MORPHOLOGY_CLASSES: Dict[str, List[str]] = {
    "BasicMorphologyFeatures": featureset_morph.BASIC,
    "EnclosingInscribingCircumscribingCircleFeature": featureset.CIRCLES,
    "ContourFeature": featureset_morph.CONTOUR,
    "ConvexHullFeature": ["CONVEX_HULL_AREA", "SOLIDITY", "CIRCULARITY"] + HEXPOLY,          # convex_hull.h:12-20
    "FractalDimensionFeature": featureset.FRACTAL,
    "GeodeticLengthThicknessFeature": featureset.GEODETIC,
    "NeighborsFeature": featureset.NEIGHBORS,
    "RoiRadiusFeature": featureset.ROI_RADIUS,
    "EllipseFittingFeature": featureset.ELLIPSE,
    "EulerNumberFeature": featureset.EULER,
    "ExtremaFeature": featureset_morph.EXTREMA,
    "ErosionPixelsFeature": featureset.EROSION,
    "CaliperFeretFeature": featureset.FERET,
    "CaliperMartinFeature": featureset.MARTIN,
    "CaliperNassensteinFeature": featureset.NASSENSTEIN,
    "ChordsFeature": featureset.CHORDS,
}
ALL_MORPHOLOGY: List[str] = [c for codes in ALL_MORPHOLOGY_CLASSES.values() for c in codes]
GROUPS_ALL_MORPH: Dict[str, List[str]] = {"*ALL_MORPHOLOGY*": ALL_MORPHOLOGY}

# featureset_morph.MORPH_REQUEST_ORDER with the three codes at their enum position: between EXTREMA_P8_Y and DIAMETER_MIN_ENCLOSING_CIRCLE
_O = featureset_morph.MORPH_REQUEST_ORDER
_H = _O.index("EXTREMA_P8_Y") + 1
assert _O[_H] == "DIAMETER_MIN_ENCLOSING_CIRCLE"
ALL_MORPH_REQUEST_ORDER: List[str] = _O[:_H] + HEXPOLY + _O[_H:]


def expand_all_morph(features: List[str]) -> Tuple[int, int, bool, List[str]]:
    """(the family mask as featureset.expand gives it, the morphology mask, whether a hexagonality / polygonality code is requested, the
    requested codes in enum order).  Everything this module does not own goes through featureset_morph.expand_morph, errors included."""
    hexpoly, rest = set(), []
    for f in features:
        key = f.strip().upper()
        if key in GROUPS_ALL_MORPH:
            for c in GROUPS_ALL_MORPH[key]:
                if c in HEXPOLY:
                    hexpoly.add(c)
                else:
                    rest.append(c)
        elif key in HEXPOLY:
            hexpoly.add(key)
        else:
            rest.append(f)
    fam_mask, mmask, codes = featureset_morph.expand_morph(rest) if rest else (0, 0, [])
    if not hexpoly and not codes:
        raise ValueError("no features requested")
    want = hexpoly | set(codes)
    return fam_mask, mmask, bool(hexpoly), [n for n in ALL_MORPH_REQUEST_ORDER if n in want]
