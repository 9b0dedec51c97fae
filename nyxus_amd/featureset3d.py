"""The `Feature3D` codes the volume entries serve (include/nyxhip.h, "volumes"): names, groups, expansion.

The reference keeps its 3-D codes in an enum of their own (featureset.h:643-) with user-facing names that start with "3"
(featureset.cpp:671-) and groups `*3D_...*` (:940-).  Two classes are served: the voxel-intensity class and the 3-D GLCM class.
`featureset.expand`, its groups and the `Nyxus` class know nothing of them.
"""
from __future__ import annotations

from typing import List, Tuple

from . import _abi

# Feature3D order (featureset.h:646-676)
INTENSITY_3D = ["3" + n for n in (
    "COV", "COVERED_IMAGE_INTENSITY_RANGE", "ENERGY", "ENTROPY", "EXCESS_KURTOSIS", "HYPERFLATNESS", "HYPERSKEWNESS", "INTEGRATED_INTENSITY",
    "INTERQUARTILE_RANGE", "KURTOSIS", "MAX", "MEAN", "MEAN_ABSOLUTE_DEVIATION", "MEDIAN", "MEDIAN_ABSOLUTE_DEVIATION", "MIN", "MODE", "P01", "P10",
    "P25", "P75", "P90", "P99", "QCOD", "RANGE", "ROBUST_MEAN", "ROBUST_MEAN_ABSOLUTE_DEVIATION", "ROOT_MEAN_SQUARED", "SKEWNESS",
    "STANDARD_DEVIATION", "STANDARD_DEVIATION_BIASED", "STANDARD_ERROR", "VARIANCE", "VARIANCE_BIASED", "UNIFORMITY", "UNIFORMITY_PIU")]
# Feature3D order (featureset.h:739-768): the angled codes, 13 directional values each
GLCM_3D_ANGLED = ["3GLCM_" + n for n in (
    "ACOR", "ASM", "CLUPROM", "CLUSHADE", "CLUTEND", "CONTRAST", "CORRELATION", "DIFAVE", "DIFENTRO", "DIFVAR", "DIS", "ENERGY", "ENTROPY", "HOM1",
    "HOM2", "ID", "IDN", "IDM", "IDMN", "INFOMEAS1", "INFOMEAS2", "IV", "JAVE", "JE", "JMAX", "JVAR", "SUMAVERAGE", "SUMENTROPY", "SUMVARIANCE",
    "VARIANCE")]
# Feature3D order (featureset.h:769-797): HOM2 has no _AVE code
GLCM_3D_AVE = ["3GLCM_" + n + "_AVE" for n in (
    "ASM", "ACOR", "CLUPROM", "CLUSHADE", "CLUTEND", "CONTRAST", "CORRELATION", "DIFAVE", "DIFENTRO", "DIFVAR", "DIS", "ENERGY", "ENTROPY", "HOM1",
    "ID", "IDN", "IDM", "IDMN", "IV", "JAVE", "JE", "INFOMEAS1", "INFOMEAS2", "VARIANCE", "JMAX", "JVAR", "SUMAVERAGE", "SUMENTROPY", "SUMVARIANCE")]
GLCM_3D = GLCM_3D_ANGLED + GLCM_3D_AVE

# the reference's spelling (featureset.cpp:941, :944); group names match in any letter case, like the 2-D groups
GROUPS_3D = {"*3D_ALL_INTENSITY*": INTENSITY_3D, "*3D_GLCM*": GLCM_3D}
ORDER_3D = INTENSITY_3D + GLCM_3D
VFAM_OF = {**{c: _abi.VFAM_INTENSITY for c in INTENSITY_3D}, **{c: _abi.VFAM_GLCM for c in GLCM_3D}}


def _refusal(names) -> str:
    return (f"feature(s) {names} are not served by the MI355X volume path. Served: the groups {sorted(GROUPS_3D)} and the individual codes of the "
            f"two classes (3COV .. 3UNIFORMITY_PIU, 3GLCM_ACOR .. 3GLCM_SUMVARIANCE_AVE); *3D_ALL*, the 3-D shape class and the other 3-D "
            "texture classes are not served")


def expand3d(features: List[str]) -> Tuple[int, List[str]]:
    """(volume mask, the requested codes in Feature3D order).  Raises ValueError for anything but the served groups and codes."""
    want, unknown = set(), []
    for f in features:
        if not isinstance(f, str):
            raise ValueError(f"feature names must be strings, got {f!r}")
        u = f.strip().upper()
        if u in GROUPS_3D:
            want.update(GROUPS_3D[u])
        elif u in VFAM_OF:
            want.add(u)
        else:
            unknown.append(f)
    if unknown:
        raise ValueError(_refusal(unknown))
    if not want:
        raise ValueError("no features requested")
    req = [c for c in ORDER_3D if c in want]
    mask = 0
    for c in req:
        mask |= VFAM_OF[c]
    return mask, req


def table_column(code: str) -> str:
    """The column of the C table that a DataFrame column shows.  The reference's buffer writer gives a Feature3D code exactly one value,
    fvals[code][0] (output_2_buffer.cpp:576-577; its GLCM expansion tests the 2-D class's codes only): an angled 3GLCM_* code is the
    value of direction shifts[0] = (1, 1, 1)."""
    return code + "_0" if code in GLCM_3D_ANGLED else code
