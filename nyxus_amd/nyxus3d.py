"""`Nyxus3D` -- the reference's volumetric Python class (src/nyx/python/nyxus/nyxus.py:923 of the reference), served by
nyxhip_featurize_volumes and nyxhip_featurize_volumes_tex (include/nyxhip.h, "volumes").

Five classes of the `Feature3D` enum are served: the voxel-intensity class (`*3D_ALL_INTENSITY*`, 36 codes), the 3-D GLCM class
(`*3D_GLCM*`, 30 angled codes and 29 `_AVE` codes), and the 3-D GLDM, NGLDM and NGTDM classes (`*3D_GLDM*` 14, `*3D_NGLDM*` 19,
`*3D_NGTDM*` 5 codes), whose grey depths and radius are metaparameters (`set_metaparam`) that start at 0 as in the reference.  The constructor takes the reference's keys and raises the reference's messages
(nyxus.py:1014-1110).  `featurize` is the in-memory face: it mirrors `Nyxus.featurize` for volumes (the reference's class has none).
The file workflows are not served: NIfTI / DICOM / z-stack ingest is outside this package.

`Nyxus3DZones` (below) is `Nyxus3D` with the 3-D GLRLM and GLSZM classes served too (nyxhip_featurize_volumes_zones), and
`Nyxus3DDistanceZones` is `Nyxus3DZones` with the 3-D GLDZM class served too (nyxhip_featurize_volumes_dzones), and `Nyxus3DShape` is
`Nyxus3DDistanceZones` with the 3-D shape class and `*3D_ALL*` served too (nyxhip_featurize_volumes_shape).
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, List, NamedTuple, Optional

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


class _Block(NamedTuple):
    """One table of the volume path, as the classes below serve it."""
    mask_attr: str                     # the attribute that holds the block's mask
    table: dict                        # code -> mask bit (featureset3d)
    names: Callable                    # (mask, settings) -> the column names of the C table
    entry: str                         # the `Context` method: entry(batch, mask, settings[, block settings], max_device_bytes=)
    settings_attr: Optional[str] = None
    new_settings: Optional[Callable] = None
    params: dict = {}                  # metaparameter key -> field of the block's settings (env_metaparams.cpp:157-239 set, :313-375 get)
    get_only: dict = {}                # keys get_metaparam alone takes
    positive: frozenset = frozenset()  # keys whose value must be a positive integer
    # (key, field, mask bit, radius field or None): the grey depths that start at 0 = unbinned, for the hint of a refused call; a class
    # whose radius is 0 reads no levels.  cap: the level cap the hint names
    depths: tuple = ()
    cap: int = 0


_VOL = _Block("_mask", featureset3d.VFAM_OF, lambda m, s: _lib.vol_column_names(m, s), "volumes_host")
# compile_feature_settings zeroes the slots (env_features.cpp:712-736)
_TEX = _Block("_tex_mask", featureset3d.VTEX_OF, lambda m, s: _lib.voltex_column_names(m), "volumes_tex_host", "_tex_settings", lambda: _abi.VolTexSettings(0, 0, 0),
              params={"3gldm/greydepth": "gldm_grey_depth", "3ngtdm/greydepth": "ngtdm_grey_depth", "3ngtdm/radius": "ngtdm_radius"},
              positive=frozenset({"3ngtdm/radius"}),
              depths=(("3gldm/greydepth", "gldm_grey_depth", _abi.VTEX_GLDM, None), ("3ngtdm/greydepth", "ngtdm_grey_depth", _abi.VTEX_NGTDM, "ngtdm_radius")),
              cap=_abi.VOLTEX_MAX_LEVELS)
# (the reference spells the GLSZM key "3glsz" where it reads it back)
_ZONE = _Block("_zone_mask", featureset3d.VZONE_OF, lambda m, s: _lib.volzone_column_names(m), "volumes_zones_host", "_zone_settings", lambda: _abi.VolZoneSettings(0, 0),
               params={"3glrlm/greydepth": "glrlm_grey_depth", "3glszm/greydepth": "glszm_grey_depth"}, get_only={"3glsz/greydepth": "glszm_grey_depth"},
               depths=(("3glrlm/greydepth", "glrlm_grey_depth", _abi.VZONE_GLRLM, None), ("3glszm/greydepth", "glszm_grey_depth", _abi.VZONE_GLSZM, None)),
               cap=_abi.VOLZONE_MAX_LEVELS)
_DZONE = _Block("_dzone_mask", featureset3d.VDZ_OF, lambda m, s: _lib.voldzone_column_names(m), "volumes_dzones_host")
_SHAPE = _Block("_shape_mask", featureset3d.VSHAPE_OF, lambda m, s: _lib.volshape_column_names(m), "volumes_shape_host")


class Nyxus3D:
    _BLOCKS = (_VOL, _TEX)                       # the tables the class serves, in the order they are computed and stand side by side
    _expand = staticmethod(featureset3d.expand3d)
    _INGEST = ("Nyxus3D.{}: NIfTI / DICOM / z-stack ingest is not served (the TIFF reader of this package decodes first pages only); "
               "assemble the volumes and call featurize()")

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
        _, self._requested = self._expand(self._features)
        for blk in self._BLOCKS:
            setattr(self, blk.mask_attr, featureset3d.mask_of(self._requested, blk.table))
            if blk.settings_attr:
                setattr(self, blk.settings_attr, blk.new_settings())
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
        names = []
        for blk in self._BLOCKS:
            mask = getattr(self, blk.mask_attr)
            if mask:
                names += blk.names(mask, self._settings)
        sel = [names.index(featureset3d.table_column(c)) for c in self._requested]
        return list(self._requested), sel

    def _metaparam(self, name: str, get: bool):
        """(settings object, field) of a metaparameter key of the served blocks."""
        for blk in self._BLOCKS:
            field = blk.params.get(name) or (get and blk.get_only.get(name))
            if field:
                return getattr(self, blk.settings_attr), field
        served = sorted(k for blk in self._BLOCKS for k in blk.params) + (sorted(k for blk in self._BLOCKS for k in blk.get_only) if get else [])
        raise ValueError(f"Invalid metaparameter name {name}: the MI355X volume path serves {served}")

    def set_metaparam(self, paramval: str):
        """Sets a feature-specific parameter, for example ``set_metaparam("3gldm/greydepth=-20")`` (nyxus.py:1111-1128).  The grey depths
        take any integer (negative: radiomics bins), ``3ngtdm/radius`` a positive one."""
        sides = str(paramval).split("=")
        if len(sides) != 2:
            raise ValueError(f"Invalid metaparameter value {paramval}: error: expecting <feature>/<parameter>=<value>")
        name, raw = sides[0].strip(), sides[1].strip()
        settings, field = self._metaparam(name, get=False)
        try:
            val = int(raw)
        except ValueError:
            val = None
        if any(name in blk.positive for blk in self._BLOCKS) and (val is None or val <= 0):
            raise ValueError(f'Invalid metaparameter value {paramval}: error: cannot parse value "{raw}" of {name}: expecting a positive integer')
        if val is None or not -2**31 <= val < 2**31:
            raise ValueError(f'Invalid metaparameter value {paramval}: error: cannot parse value "{raw}" of {name}: expecting an integer')
        setattr(settings, field, val)

    def get_metaparam(self, paramname: str) -> float:
        """The value of a feature-specific parameter, as a float like the reference's (nyxus.py:1130-1147)."""
        settings, field = self._metaparam(str(paramname).strip(), get=True)
        return float(getattr(settings, field))

    def _tables(self, b: _abi.HostBatch3D, max_device_bytes: int) -> np.ndarray:
        """The tables of the served blocks of a batch side by side, whichever the request needs (one entry each, in block order)."""
        ctx, parts = self._context(), []
        for blk in self._BLOCKS:
            mask = getattr(self, blk.mask_attr)
            if not mask:
                continue
            t = getattr(self, blk.settings_attr) if blk.settings_attr else None
            try:
                parts.append(getattr(ctx, blk.entry)(b, mask, self._settings, *([t] if t is not None else []), max_device_bytes=max_device_bytes))
            except _lib.NyxHipError as e:
                raise self._hinted(blk, mask, t, e) from e
        return parts[0] if len(parts) == 1 else np.hstack(parts)

    def _hinted(self, blk: _Block, mask: int, t, e: _lib.NyxHipError) -> _lib.NyxHipError:
        """The refusal `e` of a block's entry, with the hint at the unbinned grey depths where they explain it (else `e` itself)."""
        zero = [k for k, f, bit, radius in blk.depths if getattr(t, f) == 0 and mask & bit and not (radius and getattr(t, radius) == 0)]
        if e.code == _abi.ERR_UNSUPPORTED and zero and not self._settings.ibsi:
            return _lib.NyxHipError(e.code, f"{e.args[0]} -- a grey depth of 0 leaves the intensities unbinned: set " +
                                    " and ".join(f'set_metaparam("{k}=<levels>")' for k in zero) +
                                    f" with at most {blk.cap} levels (negative: radiomics binning)")
        return e

    def _tables_device(self, inten: np.ndarray, label: np.ndarray, max_device_bytes: int):
        """assembly="device": the volumes assembled once on the device (nyxhip_assemble_volumes), the served blocks written side by side
        into one device table through the `volumes_*_device` methods on that one resident batch, one copy back.  Returns the table, the
        labels and the volume indices of the rows."""
        import torch
        ctx = self._context()
        if label.dtype.kind != "u" or label.dtype.itemsize > 4:
            if label.size and (label.min() < 0 or label.max() > 0xFFFFFFFF):
                raise ValueError("label values must fit 32 unsigned bits")
            label = label.astype(np.uint32)
        a = ctx.assemble_volumes_host(inten, label, max_device_bytes)
        todo = [(blk, getattr(self, blk.mask_attr)) for blk in self._BLOCKS if getattr(self, blk.mask_attr)]
        widths = [len(blk.names(mask, self._settings)) for blk, mask in todo]
        ld = sum(widths)
        if a.n_roi == 0:
            return np.zeros((0, ld)), a.labels, a.volume_index
        table = torch.empty((a.n_roi, ld), dtype=torch.float64, device=torch.device("cuda", self._device))
        col = 0
        for (blk, mask), width in zip(todo, widths):
            t = getattr(self, blk.settings_attr) if blk.settings_attr else None
            try:
                getattr(ctx, blk.entry.replace("_host", "_device"))(a.batch, mask, self._settings, *([t] if t is not None else []), table.data_ptr() + 8 * col, ld)
            except _lib.NyxHipError as e:
                raise self._hinted(blk, mask, t, e) from e
            col += width
        return table.cpu().numpy(), a.labels, a.volume_index

    def featurize(self, intensity_volumes: np.ndarray, label_volumes: np.ndarray, intensity_names: Optional[list] = None,
                  label_names: Optional[list] = None, assembly: str = "host"):
        """Features of the labelled ROIs of a volume [z, y, x] or of a stack of volumes [n, z, y, x].

        Returns a DataFrame: `intensity_image`, `mask_image`, `ROI_label`, `t_index` as `Nyxus.featurize` returns them, then one column
        per requested code, rows in (volume, label) order.  The reference's table writer gives a 3-D code exactly one value
        (output_2_buffer.cpp:576-577): an angled `3GLCM_*` column is the value of direction shifts[0] = (1, 1, 1), the `_AVE` column
        the average over the 13 directions; all 13 are in the C table (nyxhip_featurize_volumes).  Values that are not finite are
        replaced by soft_nan, as the writer does.  The voxel clouds are assembled from the label volume on the host
        (`assembly="host"`, the default) or by the device label scan (`assembly="device"`: nyxhip_assemble_volumes, then every block on
        the one resident batch; the same DataFrame); no slide extrema exist in memory, so 3COVERED_IMAGE_INTENSITY_RANGE is 1
        (3d_intensity.cpp:64-65)."""
        if assembly not in ("host", "device"):
            raise ValueError(f'assembly must be "host" or "device", not {assembly!r}')
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
        if assembly == "device":
            rl = self._env.get("ram_limit", -1)
            table, labels, vol_of = self._tables_device(I, label_volumes, int(rl) << 20 if rl and rl > 0 else 0)
            if len(labels):
                table = np.ascontiguousarray(table)
                _lib.load().nyxhip_finalize_table(table.ctypes.data, table.shape[0], table.shape[1], table.shape[1], C.c_double(self._settings.soft_nan))
            else:
                table = np.zeros((0, max(sel) + 1 if sel else 0))
            return self._frame(table, labels, vol_of, cols, sel, intensity_names, label_names)
        rois, vol_of = [], []
        for v in range(nv):
            cl = clouds_from_volume(I[v], label_volumes[v])
            rois += cl
            vol_of += [v] * len(cl)
        if rois:
            b = _abi.batch3d_from_rois(rois)
            rl = self._env.get("ram_limit", -1)
            table = np.ascontiguousarray(self._tables(b, int(rl) << 20 if rl and rl > 0 else 0))
            _lib.load().nyxhip_finalize_table(table.ctypes.data, table.shape[0], table.shape[1], table.shape[1], C.c_double(self._settings.soft_nan))
            labels = b.roi_label
        else:
            table = np.zeros((0, max(sel) + 1 if sel else 0))
            labels = np.zeros(0, np.uint32)
        return self._frame(table, labels, vol_of, cols, sel, intensity_names, label_names)

    @staticmethod
    def _frame(table, labels, vol_of, cols, sel, intensity_names, label_names):
        import pandas as pd
        ti = np.asarray(vol_of, dtype=np.intp)
        df = pd.DataFrame(table[:, sel], columns=cols)
        df.insert(0, "t_index", np.zeros(len(labels)))
        df.insert(0, "ROI_label", np.asarray(labels, dtype=np.uint32))
        df.insert(0, "mask_image", np.asarray(label_names, dtype=object)[ti] if len(ti) else np.empty(0, dtype=object))
        df.insert(0, "intensity_image", np.asarray(intensity_names, dtype=object)[ti] if len(ti) else np.empty(0, dtype=object))
        return df

    def featurize_directory(self, *args, **kwargs):
        raise NotImplementedError(self._INGEST.format("featurize_directory"))

    def featurize_files(self, *args, **kwargs):
        raise NotImplementedError(self._INGEST.format("featurize_files"))


class Nyxus3DZones(Nyxus3D):
    """`Nyxus3D` with the 3-D GLRLM and GLSZM classes served too (nyxhip_featurize_volumes_zones): the groups `*3D_GLRLM*` (16 angled
    codes, 16 `_AVE` codes) and `*3D_GLSZM*` (16 codes) and their codes, beside everything `Nyxus3D` takes.  Same constructor, same
    `featurize`; the DataFrame columns stand in Feature3D order (featureset.h: the GLSZM block, then the GLRLM block, behind the NGTDM
    block), and the column of an angled `3GLRLM_*` code is direction shifts13[0] = (1, 1, 1), as the reference's table writer gives a 3-D
    code one value.  The grey depths of the two classes are the metaparameters `3glrlm/greydepth` and `3glszm/greydepth`; both start at 0
    (no binning) as in the reference, where real intensities exceed the level cap: the error names the metaparameter to set.
    `Nyxus3D` itself keeps refusing these classes."""

    _BLOCKS = (_VOL, _TEX, _ZONE)
    _expand = staticmethod(featureset3d.expand3d_zones)


class Nyxus3DDistanceZones(Nyxus3DZones):
    """`Nyxus3DZones` with the 3-D GLDZM class served too (nyxhip_featurize_volumes_dzones): the group `*3D_GLDZM*` (18 codes) and its
    codes, beside everything `Nyxus3DZones` takes.  Same constructor, same `featurize`, same metaparameters; the DataFrame columns stand
    in Feature3D order (featureset.h: the GLDZM block between the GLDM and the NGLDM blocks).  The class bins with `coarse_gray_depth`
    (or not at all in IBSI mode): the reference has no `3gldzm/greydepth` metaparameter, and this class refuses that key as
    `Nyxus3DZones` does.  A cell of level 0 forms no zone and is always a border, in every binning mode.
    `Nyxus3D` and `Nyxus3DZones` keep refusing the class; `*3D_ALL*` stays refused because the 3-D shape class is not served."""

    _BLOCKS = (_VOL, _TEX, _ZONE, _DZONE)
    _expand = staticmethod(featureset3d.expand3d_dzones)
    _INGEST = "Nyxus3DDistanceZones.{}: NIfTI / DICOM / z-stack ingest is not served; assemble the volumes and call featurize()"


class Nyxus3DShape(Nyxus3DDistanceZones):
    """`Nyxus3DDistanceZones` with the 3-D shape class served too (nyxhip_featurize_volumes_shape): the group `*3D_ALL_MORPHOLOGY*` (14
    codes, `3AREA` .. `3FLATNESS`) and its codes, beside everything `Nyxus3DDistanceZones` takes, and with them `*3D_ALL*`: every code the
    five entries serve, in Feature3D order (the enum's neighbour and moments groups are compiled out of the reference).  Same
    constructor, same `featurize`, same metaparameters; the DataFrame columns of the class stand directly behind the intensity block and in
    front of the GLCM's, as in the enum.  `3VOLUME_CONVEXHULL` and `3MESH_VOLUME` hold the exact volume of the convex hull of the centres of
    the voxels of non-zero intensity; the reference's single-ROI mode of the class is not served.
    `Nyxus3D`, `Nyxus3DZones` and `Nyxus3DDistanceZones` keep refusing the class and `*3D_ALL*`."""

    _BLOCKS = (_VOL, _TEX, _ZONE, _DZONE, _SHAPE)
    _expand = staticmethod(featureset3d.expand3d_shape)
    _INGEST = "Nyxus3DShape.{}: NIfTI / DICOM / z-stack ingest is not served; assemble the volumes and call featurize()"
