"""ctypes mirror of ``include/nyxhip.h`` (struct layouts, constants) and small
helpers that pack NumPy arrays / device pointers into a ``nyxhip_batch``.

This module only describes the C ABI; it loads nothing.  ``_lib.py`` loads the
HIP library and fails loudly when it is missing (there is no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

NYXHIP_OK = 0
ERR_UNSUPPORTED = 4
ERR_NAMES = {0: "OK", 1: "INVALID_ARG", 2: "NO_DEVICE", 3: "HIP", 4: "UNSUPPORTED", 5: "ROI_TOO_LARGE", 6: "INTERNAL"}

FAM_INTENSITY = 1 << 0
FAM_GLCM = 1 << 1
FAM_GLRLM = 1 << 2
FAM_GLSZM = 1 << 3
FAM_NGTDM = 1 << 4
FAM_GABOR = 1 << 5
FAM_ZERNIKE = 1 << 6
FAM_GLDZM = 1 << 7
FAM_GLDM = 1 << 8
FAM_NGLDM = 1 << 9
FAM_SMOMS = 1 << 10
FAM_IMOMS = 1 << 11
FAM_RADIAL = 1 << 13          # (bit 12 stays unassigned) RadialDistributionFeature (FRAC_AT_D, MEAN_FRAC, RADIAL_CV); not part of FAM_ALL
# three classes of the shape block (columns behind the intensity block); not part of FAM_ALL, bits 12 and 14 stay unassigned
FAM_FRACTAL = 1 << 15         # FractalDimensionFeature (FRACT_DIM_BOXCOUNT, FRACT_DIM_PERIMETER)
FAM_EULER = 1 << 16           # EulerNumberFeature (EULER_NUMBER)
FAM_ROI_RADIUS = 1 << 17      # RoiRadiusFeature (ROI_RADIUS_MEAN, ROI_RADIUS_MAX, ROI_RADIUS_MEDIAN)
# the three caliper classes (columns between FRACT_DIM_PERIMETER and EULER_NUMBER); not part of FAM_ALL.  They, the chords and the circle
# diameters read the ROI origin (HostBatch.origin_x / origin_y, nyxhip_featurize_batch_at)
FAM_FERET = 1 << 18           # CaliperFeretFeature (MIN_FERET_ANGLE, MAX_FERET_ANGLE, STAT_FERET_DIAM_*)
FAM_MARTIN = 1 << 19          # CaliperMartinFeature (STAT_MARTIN_DIAM_*)
FAM_NASSENSTEIN = 1 << 20     # CaliperNassensteinFeature (STAT_NASSENSTEIN_DIAM_*)
FAM_CALIPER = FAM_FERET | FAM_MARTIN | FAM_NASSENSTEIN
FAM_CHORDS = 1 << 21          # ChordsFeature (MAXCHORDS_*, ALLCHORDS_*; columns between the Nassenstein columns and EULER_NUMBER); not part
                              # of FAM_ALL; reads the ROI origin like the caliper classes
FAM_ELLIPSE = 1 << 22         # EllipseFittingFeature (MAJOR_AXIS_LENGTH .. ROUNDNESS; columns directly behind the intensity block); not part of FAM_ALL
FAM_EROSION = 1 << 23         # ErosionPixelsFeature (EROSIONS_2_VANISH, EROSIONS_2_VANISH_COMPLEMENT; behind ROUNDNESS); not part of FAM_ALL
FAM_CIRCLES = 1 << 24         # EnclosingInscribingCircumscribingCircleFeature (DIAMETER_MIN_ENCLOSING_CIRCLE, _CIRCUMSCRIBING_, _INSCRIBING_; columns
                              # directly behind EULER_NUMBER); not part of FAM_ALL; reads the ROI origin (nyxhip_featurize_batch_at)
FAM_GEODETIC = 1 << 25        # GeodeticLengthThicknessFeature (GEODETIC_LENGTH, THICKNESS; behind DIAMETER_INSCRIBING_CIRCLE); not part of FAM_ALL
FAM_NEEDS_ORIGIN = FAM_CALIPER | FAM_CHORDS | FAM_CIRCLES
FAM_NORTH_STAR = 0x7F
FAM_ALL = 0xFFF

MEM_HOST = 0
MEM_DEVICE = 1
MEM_HOST_OWN_MAPPING = 2   # nyxhip_tiles only: host arrays the caller declares mappings of their own (registered for DMA in place)

U8, U16, U32 = 1, 2, 4                       # tile element types (bytes per element)
SLIDE_MONTAGE, SLIDE_PER_TILE, SLIDE_GIVEN = 0, 1, 2

FAM_WHOLE_SLIDE = 0x3FF     # the families nyxhip_featurize_slides serves: bits 0-9, FAM_ALL without the two moment classes
MAX_GLCM_ANGLES = 4
NEIGHBOR_COLS = 9            # NYXHIP_NEIGHBOR_COLS: the table of nyxhip_neighbors_batch / _tiles (no family bit: the class relates the ROIs of an image)
HEXPOLY_COLS = 3             # NYXHIP_HEXPOLY_COLS: the table of nyxhip_hexpoly_batch / _tiles (no family bit: the class reads the neighbor count)
IH_COLS = 46                 # NYXHIP_IH_COLS: the table of nyxhip_ih_batch / _tiles (no family bit: every bit of the mask is spoken for)
IMQ_COLS = 4          # NYXHIP_IMQ_COLS: FOCUS_SCORE, LOCAL_FOCUS_SCORE, MAX_SATURATION, MIN_SATURATION
MAX_GABOR_FILTERS = 16
# NYXHIP_MORPH_*: the mask space of nyxhip_morph_batch / _tiles (no family bits: every bit of the family mask is spoken for)
MORPH_BASIC, MORPH_CONTOUR, MORPH_HULL, MORPH_EXTREMA = 1 << 0, 1 << 1, 1 << 2, 1 << 3
MORPH_ALL = 0xF
MORPH_COLS = {MORPH_BASIC: 15, MORPH_CONTOUR: 7, MORPH_HULL: 3, MORPH_EXTREMA: 16}

# NYXHIP_WS_*: the mask space of nyxhip_wsgroup_slides, the classes of the *WHOLESLIDE* group that nyxhip_featurize_slides refuses
WS_CONTOUR, WS_SMOMS, WS_IMOMS, WS_RADIAL = 1 << 0, 1 << 1, 1 << 2, 1 << 3
WS_ALL = 0xF
WS_COLS = {WS_CONTOUR: 7, WS_SMOMS: 90, WS_IMOMS: 90, WS_RADIAL: 24}
WS_BAND_PIXELS = 16384      # wsgroup_plan.h: a band of the sweep is the most whole rows with at most this many pixels (at least one row)


class Settings(C.Structure):
    """``nyxhip_settings`` (include/nyxhip.h)."""

    _fields_ = [
        ("soft_nan", C.c_double),
        ("tiny", C.c_double),
        ("grey_depth", C.c_int32),
        ("ibsi", C.c_int32),
        ("glcm_grey_depth", C.c_int32),
        ("glcm_offset", C.c_int32),
        ("glcm_n_angles", C.c_int32),
        ("glcm_angles", C.c_int32 * MAX_GLCM_ANGLES),
        ("glcm_symmetric", C.c_int32),
        ("gabor_gamma", C.c_double),
        ("gabor_sig2lam", C.c_double),
        ("gabor_f0lp", C.c_double),
        ("gabor_graythr", C.c_double),
        ("gabor_kersize", C.c_int32),
        ("gabor_n_filters", C.c_int32),
        ("gabor_f0", C.c_double * MAX_GABOR_FILTERS),
        ("gabor_theta", C.c_double * MAX_GABOR_FILTERS),
    ]


class Batch(C.Structure):
    """``nyxhip_batch`` (include/nyxhip.h)."""

    _fields_ = [
        ("n_roi", C.c_uint64),
        ("roi_label", C.c_void_p),
        ("px_offset", C.c_void_p),
        ("x", C.c_void_p),
        ("y", C.c_void_p),
        ("inten", C.c_void_p),
        ("bbox_w", C.c_void_p),
        ("bbox_h", C.c_void_p),
        ("min_inten", C.c_void_p),
        ("max_inten", C.c_void_p),
        ("slide_min", C.c_void_p),
        ("slide_max", C.c_void_p),
        ("memory", C.c_int32),
        ("max_px", C.c_uint32),
        ("max_bbox_area", C.c_uint32),
        ("max_inten_range", C.c_uint32),
        ("max_bbox_side", C.c_uint32),
    ]


class Tiles(C.Structure):
    """``nyxhip_tiles`` (include/nyxhip.h)."""

    _fields_ = [
        ("inten", C.c_void_p),
        ("label", C.c_void_p),
        ("inten_dtype", C.c_int32),
        ("label_dtype", C.c_int32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("n_tiles", C.c_uint32),
        ("memory", C.c_int32),
        ("slide_mode", C.c_int32),
        ("slide_min", C.c_void_p),
        ("slide_max", C.c_void_p),
        ("max_device_bytes", C.c_uint64),
    ]


def default_settings(coarse_gray_depth: int = 64, ibsi: bool = False) -> Settings:
    """Reference defaults: Environment::compile_feature_settings
    (/root/reference/src/nyx/env_features.cpp:713-736), glcm.cpp:8-9, gabor.cpp:14-25."""
    s = Settings()
    s.soft_nan = 0.0
    s.tiny = 1e-10
    s.grey_depth = int(coarse_gray_depth)
    s.ibsi = 1 if ibsi else 0
    s.glcm_grey_depth = int(coarse_gray_depth)
    s.glcm_offset = 1
    s.glcm_n_angles = 4
    for i, a in enumerate((0, 45, 90, 135)):
        s.glcm_angles[i] = a
    s.glcm_symmetric = 0
    s.gabor_gamma = 0.1
    s.gabor_sig2lam = 0.8
    s.gabor_f0lp = 0.1
    s.gabor_graythr = 0.025
    s.gabor_kersize = 16
    s.gabor_n_filters = 4
    # gabor.cpp:19-25 -- the pairs are declared {theta-like, f0-like} but consumed as
    # (first=f0, second=theta) at gabor.cpp:107-110; keep the consumed meaning.
    for i, (f0, th) in enumerate(((0.0, 4.0), (math.pi / 4, 16.0), (math.pi / 2, 32.0), (math.pi / 4 * 3.0, 64.0))):
        s.gabor_f0[i] = f0
        s.gabor_theta[i] = th
    return s


@dataclass
class HostBatch:
    """A host-memory ROI batch: keeps the NumPy arrays alive next to the C struct."""

    roi_label: np.ndarray
    px_offset: np.ndarray
    x: np.ndarray
    y: np.ndarray
    inten: np.ndarray
    bbox_w: np.ndarray
    bbox_h: np.ndarray
    min_inten: np.ndarray
    max_inten: np.ndarray
    slide_min: Optional[np.ndarray] = None
    slide_max: Optional[np.ndarray] = None
    origin_x: Optional[np.ndarray] = None    # [n_roi] aabb.xmin / aabb.ymin of the ROIs in their image, or None: (0, 0)
    origin_y: Optional[np.ndarray] = None
    origin_unrepresentable: bool = False     # built from ROIs whose origins do not fit uint32 (batch_from_rois)
    image_offset: Optional[np.ndarray] = None   # [n_images + 1] CSR over the rows (nyxhip_neighbors_batch), or None: one image

    def __post_init__(self):
        self.roi_label = np.ascontiguousarray(self.roi_label, np.uint32)
        self.px_offset = np.ascontiguousarray(self.px_offset, np.uint64)
        self.x = np.ascontiguousarray(self.x, np.uint16)
        self.y = np.ascontiguousarray(self.y, np.uint16)
        self.inten = np.ascontiguousarray(self.inten, np.uint32)
        self.bbox_w = np.ascontiguousarray(self.bbox_w, np.uint32)
        self.bbox_h = np.ascontiguousarray(self.bbox_h, np.uint32)
        self.min_inten = np.ascontiguousarray(self.min_inten, np.uint32)
        self.max_inten = np.ascontiguousarray(self.max_inten, np.uint32)
        if self.slide_min is not None:
            self.slide_min = np.ascontiguousarray(self.slide_min, np.float64)
            self.slide_max = np.ascontiguousarray(self.slide_max, np.float64)
        n = len(self.roi_label)
        if (self.origin_x is None) != (self.origin_y is None):
            raise ValueError("origin_x and origin_y must both be given or both None")
        if self.origin_x is not None:
            self.origin_x = np.ascontiguousarray(self.origin_x, np.uint32)
            self.origin_y = np.ascontiguousarray(self.origin_y, np.uint32)
            if len(self.origin_x) != n or len(self.origin_y) != n:
                raise ValueError("origin_x / origin_y must have n_roi entries")
        if self.image_offset is not None:
            self.image_offset = np.ascontiguousarray(self.image_offset, np.uint64)
            if len(self.image_offset) < 2 or int(self.image_offset[0]) != 0 or int(self.image_offset[-1]) != n:
                raise ValueError("image_offset must run from 0 to n_roi")
        if len(self.px_offset) != n + 1:
            raise ValueError("px_offset must have n_roi+1 entries")
        if int(self.px_offset[-1]) != len(self.inten) or len(self.x) != len(self.inten) or len(self.y) != len(self.inten):
            raise ValueError("x / y / inten length must equal px_offset[-1]")

    @property
    def n_roi(self) -> int:
        return len(self.roi_label)

    @property
    def n_px(self) -> int:
        return len(self.inten)

    def c_struct(self) -> Batch:
        b = Batch()
        b.n_roi = self.n_roi
        for name in ("roi_label", "px_offset", "x", "y", "inten", "bbox_w", "bbox_h", "min_inten", "max_inten"):
            setattr(b, name, getattr(self, name).ctypes.data)
        b.slide_min = self.slide_min.ctypes.data if self.slide_min is not None else None
        b.slide_max = self.slide_max.ctypes.data if self.slide_max is not None else None
        b.memory = MEM_HOST
        b.max_px = int(np.diff(self.px_offset.astype(np.int64)).max()) if self.n_roi else 0
        b.max_bbox_area = int((self.bbox_w.astype(np.int64) * self.bbox_h.astype(np.int64)).max()) if self.n_roi else 0
        b.max_inten_range = int((self.max_inten.astype(np.int64) - self.min_inten.astype(np.int64)).max()) if self.n_roi else 0
        b.max_bbox_side = int(max(self.bbox_w.max(), self.bbox_h.max())) if self.n_roi else 0
        return b


def batch_from_rois(rois: Sequence[dict]) -> HostBatch:
    """Builds a HostBatch from a list of dicts with keys x, y (absolute or relative
    coordinates), inten and optionally label / slide_min / slide_max.  Coordinates
    are re-based to the ROI's bounding box; min/max come from the pixels
    (what phase 1 of the reference records in LR::aux_min/aux_max,
    /root/reference/src/nyx/pixel_feed.cpp:19-43)."""
    labels, offs, xs, ys, it, bw, bh, mn, mx = [], [0], [], [], [], [], [], [], []
    ox, oy = [], []
    smin, smax = [], []
    for k, r in enumerate(rois):
        x = np.asarray(r["x"], np.int64)
        y = np.asarray(r["y"], np.int64)
        v = np.asarray(r["inten"], np.uint32)
        if len(v) == 0:
            raise ValueError("empty ROI")
        x0, y0 = x.min(), y.min()
        ox.append(int(x0))
        oy.append(int(y0))
        xs.append((x - x0).astype(np.uint16))
        ys.append((y - y0).astype(np.uint16))
        it.append(v)
        bw.append(int(x.max() - x0 + 1))
        bh.append(int(y.max() - y0 + 1))
        mn.append(int(r.get("min", v.min())))
        mx.append(int(r.get("max", v.max())))
        labels.append(int(r.get("label", k + 1)))
        offs.append(offs[-1] + len(v))
        if "slide_min" in r:
            smin.append(float(r["slide_min"]))
            smax.append(float(r["slide_max"]))
    has_slide = len(smin) == len(rois) and len(rois) > 0
    hb = HostBatch(
        np.array(labels), np.array(offs), np.concatenate(xs), np.concatenate(ys), np.concatenate(it),
        np.array(bw), np.array(bh), np.array(mn), np.array(mx),
        np.array(smin) if has_slide else None, np.array(smax) if has_slide else None)
    # the box origins (the caliper families read them).  Origins below 0 or beyond 32 bits cannot cross the ABI: the batch is marked,
    # and a call that asks for a caliper family on it is an error (Context.featurize_host) instead of rows computed at (0, 0)
    if rois and min(ox + oy) >= 0 and max(ox + oy) < 2 ** 32:
        hb.origin_x = np.array(ox, np.uint32)
        hb.origin_y = np.array(oy, np.uint32)
    else:
        hb.origin_unrepresentable = bool(rois)
    return hb


# ---- volumes (3-D): nyxhip_batch3d, the volume mask (a mask space of its own) ------------------------------------------------------
VFAM_INTENSITY = 1 << 0      # D3_VoxelIntensityFeatures: 3COV .. 3UNIFORMITY_PIU
VFAM_GLCM = 1 << 1           # D3_GLCM_feature: 30 angled codes x 13 directions, 29 _AVE codes
VFAM_ALL = 0x3
VOL_GLCM_DIRECTIONS = 13
VOL_GLCM_MAX_LEVELS = 128    # NYXHIP_VOL_GLCM_MAX_LEVELS: the co-occurrence matrix lives in LDS
VOL_MAX_CELLS = 1 << 24      # NYXHIP_VOL_MAX_CELLS: the largest box (256^3 cells)
# the texture mask of nyxhip_featurize_volumes_tex (a mask space of its own)
VTEX_GLDM = 1 << 0           # D3_GLDM_feature: 3GLDM_SDE .. 3GLDM_LDHGLE
VTEX_NGLDM = 1 << 1          # D3_NGLDM_feature: 3NGLDM_LDE .. 3NGLDM_DCENE
VTEX_NGTDM = 1 << 2          # D3_NGTDM_feature: 3NGTDM_COARSENESS .. 3NGTDM_STRENGTH
VTEX_ALL = 0x7
VOLTEX_MAX_LEVELS = 128      # NYXHIP_VOLTEX_MAX_LEVELS: the level tables live in LDS
VOLTEX_MAX_RADIUS = 3        # NYXHIP_VOLTEX_MAX_RADIUS


class VolTexSettings(C.Structure):
    """``nyxhip_voltex_settings`` (include/nyxhip.h); all three start at 0, as in the reference (env_features.cpp:712-736)."""
    _fields_ = [("gldm_grey_depth", C.c_int32), ("ngtdm_grey_depth", C.c_int32), ("ngtdm_radius", C.c_int32)]


# the zone mask of nyxhip_featurize_volumes_zones (a mask space of its own)
VZONE_GLRLM = 1 << 0         # D3_GLRLM_feature: 16 angled codes x 13 directions, 16 _AVE codes
VZONE_GLSZM = 1 << 1         # D3_GLSZM_feature: 3GLSZM_SAE .. 3GLSZM_LAHGLE
VZONE_ALL = 0x3
VOLZONE_MAX_LEVELS = 128     # NYXHIP_VOLZONE_MAX_LEVELS
VOLZONE_DIRECTIONS = 13


class VolZoneSettings(C.Structure):
    """``nyxhip_volzone_settings`` (include/nyxhip.h); both start at 0, as in the reference."""
    _fields_ = [("glrlm_grey_depth", C.c_int32), ("glszm_grey_depth", C.c_int32)]


# the distance-zone mask of nyxhip_featurize_volumes_dzones (a mask space of its own); the entry reads nyxhip_settings only
VDZ_GLDZM = 1 << 0           # D3_GLDZM_feature: 3GLDZM_SDE .. 3GLDZM_ZDE
VOLDZONE_COLS = 18
VOLDZONE_MAX_LEVELS = 128    # NYXHIP_VOLDZONE_MAX_LEVELS

# the shape mask of nyxhip_featurize_volumes_shape (a mask space of its own); the entry reads soft_nan of nyxhip_settings only
VSHAPE_MORPHOLOGY = 1 << 0   # D3_SurfaceFeature: 3AREA .. 3FLATNESS
VOLSHAPE_COLS = 14


class Batch3D(C.Structure):
    """``nyxhip_batch3d`` (include/nyxhip.h)."""

    _fields_ = [
        ("n_roi", C.c_uint64),
        ("roi_label", C.c_void_p),
        ("px_offset", C.c_void_p),
        ("x", C.c_void_p),
        ("y", C.c_void_p),
        ("z", C.c_void_p),
        ("inten", C.c_void_p),
        ("bbox_w", C.c_void_p),
        ("bbox_h", C.c_void_p),
        ("bbox_d", C.c_void_p),
        ("min_inten", C.c_void_p),
        ("max_inten", C.c_void_p),
        ("slide_min", C.c_void_p),
        ("slide_max", C.c_void_p),
        ("memory", C.c_int32),
        ("max_px", C.c_uint32),
        ("max_bbox_cells", C.c_uint32),
        ("max_inten_range", C.c_uint32),
        ("max_device_bytes", C.c_uint64),
    ]


class Volumes(C.Structure):
    """``nyxhip_volumes`` (include/nyxhip.h)."""

    _fields_ = [
        ("inten", C.c_void_p),
        ("label", C.c_void_p),
        ("inten_dtype", C.c_int32),
        ("label_dtype", C.c_int32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("depth", C.c_uint32),
        ("n_volumes", C.c_uint32),
        ("memory", C.c_int32),
        ("max_device_bytes", C.c_uint64),
    ]


def volume_dtype(dt) -> int:
    """The element type (U8 / U16 / U32) of a NumPy dtype of the volume scan."""
    dt = np.dtype(dt)
    if dt.kind != "u" or dt.itemsize not in (1, 2, 4):
        raise ValueError(f"volumes must be uint8, uint16 or uint32 arrays, not {dt}")
    return dt.itemsize


def volumes_struct(inten_ptr: int, inten_dtype: int, label_ptr: int, label_dtype: int, shape, memory: int, max_device_bytes: int = 0) -> Volumes:
    """A ``nyxhip_volumes`` over two contiguous [n, z, y, x] arrays."""
    n, d, h, w = (int(k) for k in shape)
    return Volumes(inten_ptr, label_ptr, int(inten_dtype), int(label_dtype), w, h, d, n, int(memory), int(max_device_bytes))


@dataclass
class HostBatch3D:
    """A host-memory batch of volumetric ROIs: keeps the NumPy arrays alive next to the C struct."""

    roi_label: np.ndarray
    px_offset: np.ndarray
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    inten: np.ndarray
    bbox_w: np.ndarray
    bbox_h: np.ndarray
    bbox_d: np.ndarray
    min_inten: np.ndarray
    max_inten: np.ndarray
    slide_min: Optional[np.ndarray] = None
    slide_max: Optional[np.ndarray] = None

    def __post_init__(self):
        self.roi_label = np.ascontiguousarray(self.roi_label, np.uint32)
        self.px_offset = np.ascontiguousarray(self.px_offset, np.uint64)
        for name in ("x", "y", "z"):
            setattr(self, name, np.ascontiguousarray(getattr(self, name), np.uint16))
        for name in ("inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten"):
            setattr(self, name, np.ascontiguousarray(getattr(self, name), np.uint32))
        if self.slide_min is not None:
            self.slide_min = np.ascontiguousarray(self.slide_min, np.float64)
            self.slide_max = np.ascontiguousarray(self.slide_max, np.float64)
        if len(self.px_offset) != len(self.roi_label) + 1:
            raise ValueError("px_offset must have n_roi+1 entries")
        if int(self.px_offset[-1]) != len(self.inten) or not (len(self.x) == len(self.y) == len(self.z) == len(self.inten)):
            raise ValueError("x / y / z / inten length must equal px_offset[-1]")

    @property
    def n_roi(self) -> int:
        return len(self.roi_label)

    def counts(self) -> np.ndarray:
        return np.diff(self.px_offset.astype(np.int64))

    def cells(self) -> np.ndarray:
        return self.bbox_w.astype(np.int64) * self.bbox_h.astype(np.int64) * self.bbox_d.astype(np.int64)

    def c_struct(self, stated: bool = False, max_device_bytes: int = 0) -> Batch3D:
        """stated: fill the batch extrema (max_px, max_bbox_cells, max_inten_range); otherwise the library derives them."""
        b = Batch3D()
        b.n_roi = self.n_roi
        for name in ("roi_label", "px_offset", "x", "y", "z", "inten", "bbox_w", "bbox_h", "bbox_d", "min_inten", "max_inten"):
            setattr(b, name, getattr(self, name).ctypes.data)
        b.slide_min = self.slide_min.ctypes.data if self.slide_min is not None else None
        b.slide_max = self.slide_max.ctypes.data if self.slide_max is not None else None
        b.memory = MEM_HOST
        if stated and self.n_roi:
            live = self.counts() > 0
            b.max_px = int(self.counts().max())
            b.max_bbox_cells = int(self.cells()[live].max()) if live.any() else 1
            b.max_inten_range = int((self.max_inten.astype(np.int64) - self.min_inten.astype(np.int64)).max())
        b.max_device_bytes = int(max_device_bytes)
        return b

    def select(self, idx) -> "HostBatch3D":
        """The ROIs `idx` (any order) as a batch of their own."""
        idx = [int(i) for i in idx]
        off = self.px_offset.astype(np.int64)
        sl = [slice(off[i], off[i + 1]) for i in idx]
        cat = lambda a: np.concatenate([a[s] for s in sl]) if sl else a[:0]
        pick = lambda a: a[idx] if idx else a[:0]
        return HostBatch3D(pick(self.roi_label), np.concatenate([[0], np.cumsum([s.stop - s.start for s in sl])]).astype(np.uint64),
                           cat(self.x), cat(self.y), cat(self.z), cat(self.inten), pick(self.bbox_w), pick(self.bbox_h), pick(self.bbox_d),
                           pick(self.min_inten), pick(self.max_inten),
                           pick(self.slide_min) if self.slide_min is not None else None, pick(self.slide_max) if self.slide_max is not None else None)


def batch3d_from_rois(rois: Sequence[dict]) -> HostBatch3D:
    """Builds a HostBatch3D from dicts with keys x, y, z (any origin), inten and optionally label / box (w, h, d) / origin (x0, y0, z0) /
    min / max / slide_min / slide_max.  Coordinates are re-based to the box; min / max come from the voxels.  An ROI without voxels needs
    `box`."""
    lab, offs, xs, ys, zs, it, bw, bh, bd, mn, mx, s0, s1 = [], [0], [], [], [], [], [], [], [], [], [], [], []
    for k, r in enumerate(rois):
        x, y, z = (np.asarray(r[c], np.int64) for c in "xyz")
        v = np.asarray(r["inten"], np.uint32)
        if len(v):
            x0, y0, z0 = r.get("origin", (x.min(), y.min(), z.min()))
            box = r.get("box", (x.max() - x0 + 1, y.max() - y0 + 1, z.max() - z0 + 1))
        else:
            x0 = y0 = z0 = 0
            box = r["box"]
        xs.append((x - x0).astype(np.uint16)); ys.append((y - y0).astype(np.uint16)); zs.append((z - z0).astype(np.uint16))
        it.append(v)
        bw.append(int(box[0])); bh.append(int(box[1])); bd.append(int(box[2]))
        mn.append(int(r.get("min", v.min() if len(v) else 0)))
        mx.append(int(r.get("max", v.max() if len(v) else 0)))
        lab.append(int(r.get("label", k + 1)))
        offs.append(offs[-1] + len(v))
        if "slide_min" in r:
            s0.append(float(r["slide_min"])); s1.append(float(r["slide_max"]))
    slide = len(s0) == len(rois) and len(rois) > 0
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return HostBatch3D(np.array(lab, np.uint32), np.array(offs, np.uint64), cat(xs, np.uint16), cat(ys, np.uint16), cat(zs, np.uint16), cat(it, np.uint32),
                       np.array(bw, np.uint32), np.array(bh, np.uint32), np.array(bd, np.uint32), np.array(mn, np.uint32), np.array(mx, np.uint32),
                       np.array(s0) if slide else None, np.array(s1) if slide else None)
