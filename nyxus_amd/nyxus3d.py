"""`Nyxus3D` -- the reference's volumetric Python class (src/nyx/python/nyxus/nyxus.py:923 of the reference), served by
nyxhip_featurize_volumes (include/nyxhip.h, "volumes").

Two classes of the `Feature3D` enum are served: the voxel-intensity class (`*3D_ALL_INTENSITY*`, 36 codes) and the 3-D GLCM class
(`*3D_GLCM*`, 30 angled codes and 29 `_AVE` codes).  The constructor takes the reference's keys and raises the reference's messages
(nyxus.py:1014-1110).  `featurize` is the in-memory face: it mirrors `Nyxus.featurize` for volumes (the reference's class has none).
The file workflows are not served: NIfTI / DICOM / z-stack ingest is outside this package.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np

from . import _abi, _lib, featureset3d

_VALID_KEYS = {"neighbor_distance", "pixels_per_micron", "coarse_gray_depth", "n_feature_calc_threads", "use_gpu_device", "ibsi",
               "channel_signature", "parent_channel", "child_channel", "aggregate", "dynamic_range", "min_intensity", "max_intensity",
               "ram_limit", "verbose", "anisotropy_x", "anisotropy_y", "anisotropy_z", "preserve_hu"}


def clouds_from_volume(inten: np.ndarray, label: np.ndarray):
    """The voxel clouds of one labelled volume [z, y, x], assembled on the host: a list of dicts (label, x, y, z, inten) in ascending
    label order, the voxels of an ROI in raster order (z, then y, then x)."""
    zz, yy, xx = np.nonzero(label)
    lab = label[zz, yy, xx]
    order = np.argsort(lab, kind="stable")
    lab, zz, yy, xx = lab[order], zz[order], yy[order], xx[order]
    val = inten[zz, yy, xx]
    cut = np.flatnonzero(np.diff(lab)) + 1
    starts = np.concatenate([[0], cut]).astype(np.int64) if len(lab) else np.zeros(0, np.int64)
    ends = np.concatenate([cut, [len(lab)]]).astype(np.int64) if len(lab) else np.zeros(0, np.int64)
    return [{"label": int(lab[a]), "x": xx[a:b], "y": yy[a:b], "z": zz[a:b], "inten": val[a:b]} for a, b in zip(starts, ends)]


class Nyxus3D:
    def __init__(self, features: List[str], **kwargs):
        invalid = set(kwargs) - _VALID_KEYS
        if invalid:
            print(f"Warning: unexpected keyword argument(s): {', '.join(invalid)}")
        neighbor_distance = kwargs.get("neighbor_distance", 5)
        pixels_per_micron = kwargs.get("pixels_per_micron", 1.0)
        coarse_gray_depth = kwargs.get("coarse_gray_depth", 64)
        n_threads = kwargs.get("n_feature_calc_threads", 4)
        verb = kwargs.get("verbose", 0)
        if neighbor_distance <= 0:
            raise ValueError("Neighbor distance must be greater than zero.")
        if pixels_per_micron <= 0:
            raise ValueError("Pixels per micron must be greater than zero.")
        if coarse_gray_depth <= 0:
            raise ValueError("Custom number of grayscale levels (parameter coarse_gray_depth, default=64) must be non-negative.")
        if n_threads < 1:
            raise ValueError("There must be at least one feature calculation thread.")
        if verb < 0:
            raise ValueError("verbosity must be non-negative")
        for k in ("anisotropy_x", "anisotropy_y", "anisotropy_z"):
            if kwargs.get(k, 1.0) <= 0:
                raise ValueError(f"{k} must be positive")
        if any(kwargs.get(k, 1.0) != 1.0 for k in ("anisotropy_x", "anisotropy_y", "anisotropy_z")):
            raise ValueError("anisotropy is outside the MI355X hot path (SURVEY.md section 8)")
        self._features = list(features)
        self._mask, self._requested = featureset3d.expand3d(self._features)
        # glcm_offset stays 1 and glcm_symmetric 0: the statics of the reference's 3-D GLCM class, which nothing in its Python face sets
        self._settings = _abi.default_settings(int(coarse_gray_depth), bool(kwargs.get("ibsi", False)))
        self._env = {"ram_limit": kwargs.get("ram_limit", -1)}
        self._device = max(int(kwargs.get("use_gpu_device", -1)), 0)   # the GPU is the only compute path of this package
        self._ctx: Optional[_lib.Context] = None
        self._valid_output_types = ["pandas", "arrowipc", "parquet"]

    def _context(self) -> _lib.Context:
        if self._ctx is None:
            self._ctx = _lib.Context(self._device)       # raises without a GPU / library: no CPU fallback
        return self._ctx

    def _columns(self):
        names = _lib.vol_column_names(self._mask, self._settings)
        sel = [names.index(featureset3d.table_column(c)) for c in self._requested]
        return list(self._requested), sel

    def featurize(self, intensity_volumes: np.ndarray, label_volumes: np.ndarray, intensity_names: Optional[list] = None,
                  label_names: Optional[list] = None):
        """Features of the labelled ROIs of a volume [z, y, x] or of a stack of volumes [n, z, y, x].

        Returns a DataFrame: `intensity_image`, `mask_image`, `ROI_label`, `t_index` as `Nyxus.featurize` returns them, then one column
        per requested code, rows in (volume, label) order.  The reference's table writer gives a 3-D code exactly one value
        (output_2_buffer.cpp:576-577): an angled `3GLCM_*` column is the value of direction shifts[0] = (1, 1, 1), the `_AVE` column
        the average over the 13 directions; all 13 are in the C table (nyxhip_featurize_volumes).  Values that are not finite are
        replaced by soft_nan, as the writer does.  The voxel clouds are assembled from the label volume on the host; no slide
        extrema exist in memory, so 3COVERED_IMAGE_INTENSITY_RANGE is 1 (3d_intensity.cpp:64-65)."""
        import pandas as pd
        if not isinstance(intensity_volumes, np.ndarray):
            raise ValueError("intensity_volumes parameter must be numpy.ndarray")
        if not isinstance(label_volumes, np.ndarray):
            raise ValueError("label_volumes parameter must be numpy.ndarray")
        if intensity_volumes.ndim == 3:
            if label_volumes.ndim != 3:
                raise ValueError("Both intensity and label arrays must be the same dimension")
            intensity_volumes = intensity_volumes[None]
            label_volumes = label_volumes[None]
        elif intensity_volumes.ndim != 4:
            raise ValueError("Intensity and label arrays must be 3D or 4D")
        if intensity_volumes.shape != label_volumes.shape:
            raise ValueError("Intensity and label arrays must have the same number of volumes with matching dimensions")
        nv = intensity_volumes.shape[0]
        if not intensity_names:
            intensity_names = ["Intensity" + str(i) for i in range(nv)]
        if not label_names:
            label_names = ["Segmentation" + str(i) for i in range(nv)]
        if len(intensity_names) != nv:
            raise ValueError("Number of _intensity image names_ (" + str(len(intensity_names)) + ") must be the same as the number of intensity images (" + str(nv) + ")")
        if len(label_names) != nv:
            raise ValueError("Number of segmentation names must be the same as the number of images.")
        if max(intensity_volumes.shape[1:]) > 65534:
            raise ValueError("a volume side exceeds 65534 (coordinates inside an ROI are 16-bit)")
        I = intensity_volumes
        if not np.issubdtype(I.dtype, np.unsignedinteger):      # Hounsfield-style input: shift to non-negative, then the unsigned cast
            min_raw = np.min(I) if I.size else 0
            if min_raw < 0:
                I = I - min_raw
        if I.dtype != np.uint32:
            I = I.astype(np.uint32)
        cols, sel = self._columns()
        rois, vol_of = [], []
        for v in range(nv):
            cl = clouds_from_volume(I[v], label_volumes[v])
            rois += cl
            vol_of += [v] * len(cl)
        if rois:
            b = _abi.batch3d_from_rois(rois)
            rl = self._env.get("ram_limit", -1)
            table = self._context().volumes_host(b, self._mask, self._settings, max_device_bytes=int(rl) << 20 if rl and rl > 0 else 0)
            _lib.load().nyxhip_finalize_table(table.ctypes.data, table.shape[0], table.shape[1], table.shape[1], C.c_double(self._settings.soft_nan))
            labels = b.roi_label
        else:
            table = np.zeros((0, max(sel) + 1 if sel else 0))
            labels = np.zeros(0, np.uint32)
        ti = np.asarray(vol_of, dtype=np.intp)
        df = pd.DataFrame(table[:, sel], columns=cols)
        df.insert(0, "t_index", np.zeros(len(labels)))
        df.insert(0, "ROI_label", np.asarray(labels, dtype=np.uint32))
        df.insert(0, "mask_image", np.asarray(label_names, dtype=object)[ti] if len(ti) else np.empty(0, dtype=object))
        df.insert(0, "intensity_image", np.asarray(intensity_names, dtype=object)[ti] if len(ti) else np.empty(0, dtype=object))
        return df

    def featurize_directory(self, *args, **kwargs):
        raise NotImplementedError("Nyxus3D.featurize_directory: NIfTI / DICOM / z-stack ingest is not served (the TIFF reader of this package "
                                  "decodes first pages only); assemble the volumes and call featurize()")

    def featurize_files(self, *args, **kwargs):
        raise NotImplementedError("Nyxus3D.featurize_files: NIfTI / DICOM / z-stack ingest is not served (the TIFF reader of this package "
                                  "decodes first pages only); assemble the volumes and call featurize()")
