"""The `Feature3D` codes the volume entries serve (include/nyxhip.h, "volumes"): names, groups, expansion.

The reference keeps its 3-D codes in an enum of their own (featureset.h:643-) with user-facing names that start with "3"
(featureset.cpp:671-) and groups `*3D_...*` (:940-).  Five classes are served: the voxel-intensity class and the 3-D GLCM class by the
volume mask of nyxhip_featurize_volumes, the 3-D GLDM, NGLDM and NGTDM classes by the texture mask of nyxhip_featurize_volumes_tex.
`featureset.expand`, its groups and the `Nyxus` class know nothing of them.  Two more classes, the 3-D GLRLM and GLSZM, are served by the
zone mask of nyxhip_featurize_volumes_zones through `expand3d_zones` and `Nyxus3DZones`; `expand3d` and `Nyxus3D` refuse them.  The last
texture class, the 3-D GLDZM, is served by the distance-zone mask of nyxhip_featurize_volumes_dzones through `expand3d_dzones` and
`Nyxus3DDistanceZones`; the other expansions and classes refuse it.  The shape class (14 codes, `*3D_ALL_MORPHOLOGY*`) is served by the
shape mask of nyxhip_featurize_volumes_shape through `expand3d_shape` and `Nyxus3DShape`, and with it `*3D_ALL*`.
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
# Feature3D order (featureset.cpp:827-840, :911-929, :931-935); the enum has the GLDM block before the NGLDM and NGTDM blocks
GLDM_3D = ["3GLDM_" + n for n in ("SDE", "LDE", "GLN", "DN", "DNN", "GLV", "DV", "DE", "LGLE", "HGLE", "SDLGLE", "SDHGLE", "LDLGLE", "LDHGLE")]
NGLDM_3D = ["3NGLDM_" + n for n in ("LDE", "HDE", "LGLCE", "HGLCE", "LDLGLE", "LDHGLE", "HDLGLE", "HDHGLE", "GLNU", "GLNUN", "DCNU", "DCNUN", "DCP", "GLM",
                                    "GLV", "DCM", "DCV", "DCENT", "DCENE")]
NGTDM_3D = ["3NGTDM_" + n for n in ("COARSENESS", "CONTRAST", "BUSYNESS", "COMPLEXITY", "STRENGTH")]

# Feature3D order (featureset.h:863-914, names featureset.cpp:861-909): in the enum the GLSZM block and then the GLRLM block (angled codes,
# then the _AVE codes) stand behind the NGTDM block.  Served by Nyxus3DZones / expand3d_zones only (the zone mask of
# nyxhip_featurize_volumes_zones); expand3d refuses them.
GLSZM_3D = ["3GLSZM_" + n for n in ("SAE", "LAE", "GLN", "GLNN", "SZN", "SZNN", "ZP", "GLV", "ZV", "ZE", "LGLZE", "HGLZE", "SALGLE", "SAHGLE", "LALGLE", "LAHGLE")]
GLRLM_3D_ANGLED = ["3GLRLM_" + n for n in ("SRE", "LRE", "GLN", "GLNN", "RLN", "RLNN", "RP", "GLV", "RV", "RE", "LGLRE", "HGLRE", "SRLGLE", "SRHGLE", "LRLGLE",
                                           "LRHGLE")]
GLRLM_3D_AVE = [c + "_AVE" for c in GLRLM_3D_ANGLED]
GLRLM_3D = GLRLM_3D_ANGLED + GLRLM_3D_AVE

# the reference's spelling (featureset.cpp:941, :944); group names match in any letter case, like the 2-D groups
GROUPS_3D = {"*3D_ALL_INTENSITY*": INTENSITY_3D, "*3D_GLCM*": GLCM_3D, "*3D_GLDM*": GLDM_3D, "*3D_NGLDM*": NGLDM_3D, "*3D_NGTDM*": NGTDM_3D}
ORDER_3D = INTENSITY_3D + GLCM_3D + GLDM_3D + NGLDM_3D + NGTDM_3D
# a code belongs to one of the two mask spaces: the volume mask (VFAM_OF, 0 for a texture code) or the texture mask (VTEX_OF)
VTEX_OF = {**{c: _abi.VTEX_GLDM for c in GLDM_3D}, **{c: _abi.VTEX_NGLDM for c in NGLDM_3D}, **{c: _abi.VTEX_NGTDM for c in NGTDM_3D}}
GROUPS_3D_ZONES = {"*3D_GLRLM*": GLRLM_3D, "*3D_GLSZM*": GLSZM_3D}
ORDER_3D_ZONES = ORDER_3D + GLSZM_3D + GLRLM_3D
VZONE_OF = {**{c: _abi.VZONE_GLRLM for c in GLRLM_3D}, **{c: _abi.VZONE_GLSZM for c in GLSZM_3D}}
# Feature3D order (featureset.h:815-833, names featureset.cpp:842-859): in the enum the GLDZM block stands between the GLDM and the NGLDM
# blocks.  Served by Nyxus3DDistanceZones / expand3d_dzones only (the distance-zone mask of nyxhip_featurize_volumes_dzones); expand3d
# and expand3d_zones refuse it.
GLDZM_3D = ["3GLDZM_" + n for n in ("SDE", "LDE", "LGLZE", "HGLZE", "SDLGLE", "SDHGLE", "LDLGLE", "LDHGLE", "GLNU", "GLNUN", "ZDNU", "ZDNUN", "ZP", "GLM", "GLV", "ZDM",
                                    "ZDV", "ZDE")]
GROUPS_3D_DZONES = {"*3D_GLDZM*": GLDZM_3D}
ORDER_3D_DZONES = INTENSITY_3D + GLCM_3D + GLDM_3D + GLDZM_3D + NGLDM_3D + NGTDM_3D + GLSZM_3D + GLRLM_3D
VDZ_OF = {c: _abi.VDZ_GLDZM for c in GLDZM_3D}
# Feature3D order (featureset.h:678-693, names featureset.cpp:712-725): in the enum the shape block stands directly behind the intensity
# block.  Served by Nyxus3DShape / expand3d_shape only (the shape mask of nyxhip_featurize_volumes_shape); the other expansions refuse
# it.  *3D_ALL* is the union of what the five entries serve, in enum order: the enum's neighbour and moments groups are compiled out of
# the reference (#if 0) and single codes of theirs do not exist.
SHAPE_3D = ["3" + n for n in ("AREA", "AREA_2_VOLUME", "COMPACTNESS1", "COMPACTNESS2", "MESH_VOLUME", "SPHERICAL_DISPROPORTION", "SPHERICITY", "VOLUME_CONVEXHULL",
                              "VOXEL_VOLUME", "MAJOR_AXIS_LEN", "MINOR_AXIS_LEN", "LEAST_AXIS_LEN", "ELONGATION", "FLATNESS")]
ORDER_3D_SHAPE = INTENSITY_3D + SHAPE_3D + GLCM_3D + GLDM_3D + GLDZM_3D + NGLDM_3D + NGTDM_3D + GLSZM_3D + GLRLM_3D
GROUPS_3D_SHAPE = {"*3D_ALL_MORPHOLOGY*": SHAPE_3D, "*3D_ALL*": ORDER_3D_SHAPE}
VSHAPE_OF = {c: _abi.VSHAPE_MORPHOLOGY for c in SHAPE_3D}
VFAM_OF = {**{c: _abi.VFAM_INTENSITY for c in INTENSITY_3D}, **{c: _abi.VFAM_GLCM for c in GLCM_3D}, **{c: 0 for c in VTEX_OF}}


def _refusal(names) -> str:
    return (f"feature(s) {names} are not served by the MI355X volume path. Served: the groups {sorted(GROUPS_3D)} and the individual codes of the "
            f"five classes (3COV .. 3UNIFORMITY_PIU, 3GLCM_ACOR .. 3GLCM_SUMVARIANCE_AVE, 3GLDM_SDE .. 3GLDM_LDHGLE, 3NGLDM_LDE .. 3NGLDM_DCENE, "
            "3NGTDM_COARSENESS .. 3NGTDM_STRENGTH); *3D_ALL*, the 3-D shape class and the 3-D GLRLM, GLSZM and GLDZM classes are not served. "
            "The 3-D GLRLM and GLSZM classes are served by Nyxus3DZones (featureset3d.expand3d_zones), the 3-D GLDZM class by "
            "Nyxus3DDistanceZones (featureset3d.expand3d_dzones)")


# what an expansion serves: (groups, code -> mask bit) per tier, and the Feature3D order of all its codes
_TIERS_3D = [(GROUPS_3D, VFAM_OF)]
_TIERS_3D_ZONES = _TIERS_3D + [(GROUPS_3D_ZONES, VZONE_OF)]
_TIERS_3D_DZONES = _TIERS_3D_ZONES + [(GROUPS_3D_DZONES, VDZ_OF)]
_TIERS_3D_SHAPE = _TIERS_3D_DZONES + [(GROUPS_3D_SHAPE, VSHAPE_OF)]


def _expand(features: List[str], tiers, order: List[str]) -> Tuple[int, List[str]]:
    want, unknown = set(), []
    for f in features:
        if not isinstance(f, str):
            raise ValueError(f"feature names must be strings, got {f!r}")
        u = f.strip().upper()
        for groups, table in tiers:
            if u in groups:
                want.update(groups[u])
                break
            if u in table:
                want.add(u)
                break
        else:
            unknown.append(f)
    if unknown:
        raise ValueError(_refusal(unknown))
    if not want:
        raise ValueError("no features requested")
    req = [c for c in order if c in want]
    return mask_of(req, VFAM_OF), req


def mask_of(codes: List[str], table) -> int:
    """The bits of `table` (code -> mask bit) that serve the codes among `codes`; 0: none."""
    m = 0
    for c in codes:
        m |= table.get(c, 0)
    return m


def expand3d(features: List[str]) -> Tuple[int, List[str]]:
    """(volume mask, the requested codes in Feature3D order).  Raises ValueError for anything but the served groups and codes.  The
    volume mask is 0 when only texture codes are asked for; their mask is tex_mask(codes)."""
    return _expand(features, _TIERS_3D, ORDER_3D)


def expand3d_zones(features: List[str]) -> Tuple[int, List[str]]:
    """expand3d with the groups *3D_GLRLM*, *3D_GLSZM* and their codes served too: (volume mask, the requested codes in Feature3D
    order).  The texture mask is tex_mask(codes), the zone mask zone_mask(codes)."""
    return _expand(features, _TIERS_3D_ZONES, ORDER_3D_ZONES)


def expand3d_dzones(features: List[str]) -> Tuple[int, List[str]]:
    """expand3d_zones with the group *3D_GLDZM* and its codes served too: (volume mask, the requested codes in Feature3D order).  The
    distance-zone mask is dzone_mask(codes)."""
    return _expand(features, _TIERS_3D_DZONES, ORDER_3D_DZONES)


def expand3d_shape(features: List[str]) -> Tuple[int, List[str]]:
    """expand3d_dzones with the groups *3D_ALL_MORPHOLOGY*, *3D_ALL* and the 14 shape codes served too: (volume mask, the requested codes in
    Feature3D order).  The shape mask is shape_mask(codes)."""
    return _expand(features, _TIERS_3D_SHAPE, ORDER_3D_SHAPE)


def shape_mask(codes: List[str]) -> int:
    """The shape mask (nyxhip_featurize_volumes_shape) that serves the shape codes among `codes`; 0: none."""
    return mask_of(codes, VSHAPE_OF)


def dzone_mask(codes: List[str]) -> int:
    """The distance-zone mask (nyxhip_featurize_volumes_dzones) that serves the GLDZM codes among `codes`; 0: none."""
    return mask_of(codes, VDZ_OF)


def zone_mask(codes: List[str]) -> int:
    """The zone mask (nyxhip_featurize_volumes_zones) that serves the GLRLM / GLSZM codes among `codes`; 0: none."""
    return mask_of(codes, VZONE_OF)


def tex_mask(codes: List[str]) -> int:
    """The texture mask (nyxhip_featurize_volumes_tex) that serves the GLDM / NGLDM / NGTDM codes among `codes`; 0: none."""
    return mask_of(codes, VTEX_OF)


def table_column(code: str) -> str:
    """The column of the C table that a DataFrame column shows.  The reference's buffer writer gives a Feature3D code exactly one value,
    fvals[code][0] (output_2_buffer.cpp:576-577; its GLCM expansion tests the 2-D class's codes only): an angled 3GLCM_* code is the
    value of direction shifts[0] = (1, 1, 1), and so is an angled 3GLRLM_* code (shifts13[0])."""
    return code + "_0" if code in GLCM_3D_ANGLED or code in GLRLM_3D_ANGLED else code
