"""Loader and thin Python face of the C ABI (``include/nyxhip.h``).

The HIP library is the product: if ``libnyxhip.so`` is missing or no GPU is
present this module raises -- there is no CPU fallback on the product path.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
import sys
import weakref
from typing import List, NamedTuple, Optional

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# NYXHIP_LIB selects another build of the same ABI (e.g. the stamped diagnostic build)
LIB_PATH = os.environ.get("NYXHIP_LIB") or os.path.join(_HERE, "libnyxhip.so")

# every symbol include/nyxhip.h declares
ABI_SYMBOLS = [
    "nyxhip_abi_version", "nyxhip_default_settings", "nyxhip_init", "nyxhip_destroy", "nyxhip_last_error",
    "nyxhip_set_stream", "nyxhip_n_columns", "nyxhip_column_name", "nyxhip_featurize_batch",
    "nyxhip_featurize_batch_async", "nyxhip_sync", "nyxhip_finalize_table", "nyxhip_featurize_tile", "nyxhip_featurize_tiles",
    "nyxhip_timing_enable", "nyxhip_timing_reset", "nyxhip_timing_get",
    "nyxhip_featurize_tiles_v2", "nyxhip_fetch_result", "nyxhip_featurize_tiles_sharded", "nyxhip_fetch_result_sharded",
    "nyxhip_launch_report", "nyxhip_debug_roi_words", "nyxhip_featurize_batch_at", "nyxhip_featurize_batch_async_at",
    "nyxhip_neighbor_column_name", "nyxhip_neighbors_batch", "nyxhip_neighbors_tiles",
    "nyxhip_ih_column_name", "nyxhip_ih_batch", "nyxhip_ih_tiles",
    "nyxhip_featurize_slides",
    "nyxhip_imq_column_name", "nyxhip_imq_batch", "nyxhip_imq_tiles", "nyxhip_imq_slides",
    "nyxhip_wsgroup_n_columns", "nyxhip_wsgroup_column_name", "nyxhip_wsgroup_slides",
    "nyxhip_vol_n_columns", "nyxhip_vol_column_name", "nyxhip_featurize_volumes",
    "nyxhip_voltex_n_columns", "nyxhip_voltex_column_name", "nyxhip_featurize_volumes_tex",
    "nyxhip_volzone_n_columns", "nyxhip_volzone_column_name", "nyxhip_featurize_volumes_zones",
    "nyxhip_voldzone_n_columns", "nyxhip_voldzone_column_name", "nyxhip_featurize_volumes_dzones",
    "nyxhip_vshape_n_columns", "nyxhip_vshape_column_name", "nyxhip_featurize_volumes_shape",
    "nyxhip_morph_n_columns", "nyxhip_morph_column_name", "nyxhip_morph_batch", "nyxhip_morph_tiles",
    "nyxhip_hexpoly_column_name", "nyxhip_hexpoly_batch", "nyxhip_hexpoly_tiles",
    "nyxhip_assemble_volumes", "nyxhip_assembled_rows", "nyxhip_release_volumes",
]


class NyxHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"nyxhip error {code} ({_abi.ERR_NAMES.get(code, '?')}): {msg}")
        self.code = code


_lib = None


def load() -> C.CDLL:
    """dlopen()s libnyxhip.so and declares the prototypes.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C nyxus_amd/csrc).  The MI355X path has no CPU fallback.")
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64 (same SONAME as
    # /opt/rocm's).  If libnyxhip.so pulled in the system copy first and torch loaded its own later,
    # the second runtime would see no GPU.  Importing torch first makes the dynamic linker resolve
    # libnyxhip.so against the already-loaded copy.  (Pure C/C++ users of the ABI are unaffected.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    P = C.POINTER
    lib.nyxhip_abi_version.restype = C.c_int
    lib.nyxhip_default_settings.argtypes = [P(_abi.Settings)]
    lib.nyxhip_default_settings.restype = None
    lib.nyxhip_init.argtypes = [C.c_int, P(C.c_void_p)]
    lib.nyxhip_init.restype = C.c_int
    lib.nyxhip_destroy.argtypes = [C.c_void_p]
    lib.nyxhip_destroy.restype = None
    lib.nyxhip_last_error.argtypes = [C.c_void_p]
    lib.nyxhip_last_error.restype = C.c_char_p
    lib.nyxhip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.nyxhip_set_stream.restype = C.c_int
    lib.nyxhip_n_columns.argtypes = [C.c_uint32, P(_abi.Settings)]
    lib.nyxhip_n_columns.restype = C.c_int
    lib.nyxhip_column_name.argtypes = [C.c_uint32, P(_abi.Settings), C.c_int, C.c_char_p, C.c_size_t]
    lib.nyxhip_column_name.restype = C.c_int
    for name in ("nyxhip_featurize_batch", "nyxhip_featurize_batch_async"):
        f = getattr(lib, name)
        f.argtypes = [C.c_void_p, P(_abi.Batch), C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_size_t]
        f.restype = C.c_int
    for name in ("nyxhip_featurize_batch_at", "nyxhip_featurize_batch_async_at"):
        f = getattr(lib, name)
        f.argtypes = [C.c_void_p, P(_abi.Batch), C.c_void_p, C.c_void_p, C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_size_t]
        f.restype = C.c_int
    lib.nyxhip_sync.argtypes = [C.c_void_p]
    lib.nyxhip_sync.restype = C.c_int
    lib.nyxhip_finalize_table.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double]
    lib.nyxhip_finalize_table.restype = None
    lib.nyxhip_featurize_tile.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32,
                                          C.c_uint32, C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_uint64,
                                          C.c_void_p, C.c_size_t, P(C.c_uint64)]
    lib.nyxhip_featurize_tile.restype = C.c_int
    lib.nyxhip_featurize_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32,
                                           C.c_uint32, C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_void_p, C.c_uint64,
                                           C.c_void_p, C.c_size_t, P(C.c_uint64)]
    lib.nyxhip_featurize_tiles.restype = C.c_int
    lib.nyxhip_featurize_tiles_v2.argtypes = [C.c_void_p, P(_abi.Tiles), C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_void_p, C.c_uint64,
                                              C.c_void_p, C.c_size_t, P(C.c_uint64)]
    lib.nyxhip_featurize_tiles_v2.restype = C.c_int
    lib.nyxhip_fetch_result.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.nyxhip_fetch_result.restype = C.c_int
    lib.nyxhip_featurize_tiles_sharded.argtypes = [P(C.c_void_p), C.c_int, P(_abi.Tiles), C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_void_p,
                                                   C.c_uint64, C.c_void_p, C.c_size_t, P(C.c_uint64)]
    lib.nyxhip_featurize_tiles_sharded.restype = C.c_int
    lib.nyxhip_fetch_result_sharded.argtypes = [P(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.nyxhip_fetch_result_sharded.restype = C.c_int
    lib.nyxhip_timing_enable.argtypes = [C.c_void_p, C.c_int]
    lib.nyxhip_timing_enable.restype = C.c_int
    lib.nyxhip_timing_reset.argtypes = [C.c_void_p]
    lib.nyxhip_timing_reset.restype = C.c_int
    lib.nyxhip_timing_get.argtypes = [C.c_void_p, P(C.c_double), P(C.c_uint64)]
    lib.nyxhip_timing_get.restype = C.c_int
    if hasattr(lib, "nyxhip_neighbors_batch"):   # (absent from older builds of the ABI selected through NYXHIP_LIB for A/B runs)
        lib.nyxhip_neighbor_column_name.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        lib.nyxhip_neighbor_column_name.restype = C.c_int
        lib.nyxhip_neighbors_batch.argtypes = [C.c_void_p, P(_abi.Batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, P(_abi.Settings),
                                               C.c_void_p, C.c_size_t]
        lib.nyxhip_neighbors_batch.restype = C.c_int
        lib.nyxhip_neighbors_tiles.argtypes = [C.c_void_p, P(_abi.Tiles), C.c_int32, P(_abi.Settings), C.c_void_p, C.c_void_p, C.c_uint64,
                                               C.c_void_p, C.c_size_t, P(C.c_uint64)]
        lib.nyxhip_neighbors_tiles.restype = C.c_int
    if hasattr(lib, "nyxhip_ih_batch"):          # (absent from older builds of the ABI selected through NYXHIP_LIB for A/B runs)
        lib.nyxhip_ih_column_name.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        lib.nyxhip_ih_column_name.restype = C.c_int
        lib.nyxhip_ih_batch.argtypes = [C.c_void_p, P(_abi.Batch), P(_abi.Settings), C.c_void_p, C.c_size_t]
        lib.nyxhip_ih_batch.restype = C.c_int
        lib.nyxhip_ih_tiles.argtypes = [C.c_void_p, P(_abi.Tiles), P(_abi.Settings), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t,
                                        P(C.c_uint64)]
        lib.nyxhip_ih_tiles.restype = C.c_int
    if hasattr(lib, "nyxhip_imq_batch"):         # (absent from older builds of the ABI selected through NYXHIP_LIB for A/B runs)
        lib.nyxhip_imq_column_name.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        lib.nyxhip_imq_column_name.restype = C.c_int
        lib.nyxhip_imq_batch.argtypes = [C.c_void_p, P(_abi.Batch), P(_abi.Settings), C.c_void_p, C.c_size_t]
        lib.nyxhip_imq_batch.restype = C.c_int
        lib.nyxhip_imq_tiles.argtypes = [C.c_void_p, P(_abi.Tiles), P(_abi.Settings), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t,
                                         P(C.c_uint64)]
        lib.nyxhip_imq_tiles.restype = C.c_int
        lib.nyxhip_imq_slides.argtypes = [C.c_void_p, P(_abi.Tiles), P(_abi.Settings), C.c_void_p, C.c_size_t]
        lib.nyxhip_imq_slides.restype = C.c_int
    if hasattr(lib, "nyxhip_wsgroup_slides"):
        lib.nyxhip_wsgroup_n_columns.argtypes = [C.c_uint32]
        lib.nyxhip_wsgroup_n_columns.restype = C.c_int
        lib.nyxhip_wsgroup_column_name.argtypes = [C.c_uint32, C.c_int, C.c_char_p, C.c_size_t]
        lib.nyxhip_wsgroup_column_name.restype = C.c_int
        lib.nyxhip_wsgroup_slides.argtypes = [C.c_void_p, P(_abi.Tiles), C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_size_t]
        lib.nyxhip_wsgroup_slides.restype = C.c_int
    if hasattr(lib, "nyxhip_featurize_volumes"):  # (absent from older builds of the ABI selected through NYXHIP_LIB for A/B runs)
        lib.nyxhip_vol_n_columns.argtypes = [C.c_uint32, P(_abi.Settings)]
        lib.nyxhip_vol_n_columns.restype = C.c_int
        lib.nyxhip_vol_column_name.argtypes = [C.c_uint32, P(_abi.Settings), C.c_int, C.c_char_p, C.c_size_t]
        lib.nyxhip_vol_column_name.restype = C.c_int
        lib.nyxhip_featurize_volumes.argtypes = [C.c_void_p, P(_abi.Batch3D), C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_size_t]
        lib.nyxhip_featurize_volumes.restype = C.c_int
    if hasattr(lib, "nyxhip_featurize_volumes_tex"):
        lib.nyxhip_voltex_n_columns.argtypes = [C.c_uint32]
        lib.nyxhip_voltex_n_columns.restype = C.c_int
        lib.nyxhip_voltex_column_name.argtypes = [C.c_uint32, C.c_int, C.c_char_p, C.c_size_t]
        lib.nyxhip_voltex_column_name.restype = C.c_int
        lib.nyxhip_featurize_volumes_tex.argtypes = [C.c_void_p, P(_abi.Batch3D), C.c_uint32, P(_abi.Settings), P(_abi.VolTexSettings), C.c_void_p, C.c_size_t]
        lib.nyxhip_volzone_n_columns.argtypes = [C.c_uint32]
        lib.nyxhip_volzone_n_columns.restype = C.c_int
        lib.nyxhip_volzone_column_name.argtypes = [C.c_uint32, C.c_int, C.c_char_p, C.c_size_t]
        lib.nyxhip_volzone_column_name.restype = C.c_int
        lib.nyxhip_featurize_volumes_zones.argtypes = [C.c_void_p, P(_abi.Batch3D), C.c_uint32, P(_abi.Settings), P(_abi.VolZoneSettings), C.c_void_p, C.c_size_t]
        lib.nyxhip_featurize_volumes_tex.restype = C.c_int
    if hasattr(lib, "nyxhip_featurize_volumes_dzones"):
        lib.nyxhip_voldzone_n_columns.argtypes = [C.c_uint32]
        lib.nyxhip_voldzone_n_columns.restype = C.c_int
        lib.nyxhip_voldzone_column_name.argtypes = [C.c_uint32, C.c_int, C.c_char_p, C.c_size_t]
        lib.nyxhip_voldzone_column_name.restype = C.c_int
        lib.nyxhip_featurize_volumes_dzones.argtypes = [C.c_void_p, P(_abi.Batch3D), C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_size_t]
        lib.nyxhip_featurize_volumes_dzones.restype = C.c_int
    if hasattr(lib, "nyxhip_featurize_volumes_shape"):
        lib.nyxhip_vshape_n_columns.argtypes = [C.c_uint32]
        lib.nyxhip_vshape_n_columns.restype = C.c_int
        lib.nyxhip_vshape_column_name.argtypes = [C.c_uint32, C.c_int, C.c_char_p, C.c_size_t]
        lib.nyxhip_vshape_column_name.restype = C.c_int
        lib.nyxhip_featurize_volumes_shape.argtypes = [C.c_void_p, P(_abi.Batch3D), C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_size_t]
        lib.nyxhip_featurize_volumes_shape.restype = C.c_int
    if hasattr(lib, "nyxhip_assemble_volumes"):
        lib.nyxhip_assemble_volumes.argtypes = [C.c_void_p, P(_abi.Volumes), P(_abi.Batch3D), P(C.c_void_p)]
        lib.nyxhip_assemble_volumes.restype = C.c_int
        lib.nyxhip_assembled_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        lib.nyxhip_assembled_rows.restype = C.c_int
        lib.nyxhip_release_volumes.argtypes = [C.c_void_p]
        lib.nyxhip_release_volumes.restype = C.c_int
    if hasattr(lib, "nyxhip_morph_batch"):      # (absent from older builds of the ABI selected through NYXHIP_LIB for A/B runs)
        lib.nyxhip_morph_n_columns.argtypes = [C.c_uint32]
        lib.nyxhip_morph_n_columns.restype = C.c_int
        lib.nyxhip_morph_column_name.argtypes = [C.c_uint32, C.c_int, C.c_char_p, C.c_size_t]
        lib.nyxhip_morph_column_name.restype = C.c_int
        lib.nyxhip_morph_batch.argtypes = [C.c_void_p, P(_abi.Batch), C.c_void_p, C.c_void_p, C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_size_t]
        lib.nyxhip_morph_batch.restype = C.c_int
        lib.nyxhip_morph_tiles.argtypes = [C.c_void_p, P(_abi.Tiles), C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_void_p, C.c_uint64,
                                           C.c_void_p, C.c_size_t, P(C.c_uint64)]
        lib.nyxhip_morph_tiles.restype = C.c_int
    if hasattr(lib, "nyxhip_hexpoly_batch"):     # (absent from older builds of the ABI selected through NYXHIP_LIB for A/B runs)
        lib.nyxhip_hexpoly_column_name.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        lib.nyxhip_hexpoly_column_name.restype = C.c_int
        lib.nyxhip_hexpoly_batch.argtypes = [C.c_void_p, P(_abi.Batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, P(_abi.Settings),
                                             C.c_void_p, C.c_size_t]
        lib.nyxhip_hexpoly_batch.restype = C.c_int
        lib.nyxhip_hexpoly_tiles.argtypes = [C.c_void_p, P(_abi.Tiles), C.c_int32, P(_abi.Settings), C.c_void_p, C.c_void_p, C.c_uint64,
                                             C.c_void_p, C.c_size_t, P(C.c_uint64)]
        lib.nyxhip_hexpoly_tiles.restype = C.c_int
    if hasattr(lib, "nyxhip_featurize_slides"):  # (absent from older builds of the ABI selected through NYXHIP_LIB for A/B runs)
        lib.nyxhip_featurize_slides.argtypes = [C.c_void_p, P(_abi.Tiles), C.c_uint32, P(_abi.Settings), C.c_void_p, C.c_size_t]
        lib.nyxhip_featurize_slides.restype = C.c_int
    if hasattr(lib, "nyxhip_launch_report"):     # (absent from older builds of the ABI selected through NYXHIP_LIB for A/B runs)
        lib.nyxhip_launch_report.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        lib.nyxhip_launch_report.restype = C.c_int
    if hasattr(lib, "nyxhip_debug_roi_words"):   # (absent from older builds of the ABI selected through NYXHIP_LIB for A/B runs)
        lib.nyxhip_debug_roi_words.argtypes = [C.c_void_p, C.c_uint64, P(C.c_uint64), P(C.c_uint64)]
        lib.nyxhip_debug_roi_words.restype = C.c_int
    _lib = lib
    return lib


def _catalogue(n_columns, column_name, lead: tuple, column_noun: str, mask_noun: Optional[str] = None) -> List[str]:
    """The names of an n_columns / column_name pair of the library.  `lead`: the arguments ahead of the column index (mask, settings, or
    nothing); `n_columns`: the C function, or the count itself; the nouns are those of the error texts (`mask_noun`: of a refused mask)."""
    n = n_columns(*lead) if callable(n_columns) else n_columns
    if n < 0 and mask_noun:
        raise NyxHipError(1, f"bad {mask_noun} {lead[0]:#x}")
    buf = C.create_string_buffer(128)
    out = []
    for i in range(n):
        rc = column_name(*lead, i, buf, 128)
        if rc != 0:
            raise NyxHipError(rc, f"{column_noun} {i}")
        out.append(buf.value.decode())
    return out


def column_names(mask: int, s: _abi.Settings) -> List[str]:
    return _catalogue(load().nyxhip_n_columns, load().nyxhip_column_name, (mask, C.byref(s)), "column")


def neighbor_column_names() -> List[str]:
    """The nine columns of nyxhip_neighbors_batch / _tiles, enum order."""
    return _catalogue(_abi.NEIGHBOR_COLS, load().nyxhip_neighbor_column_name, (), "neighbor column")


def hexpoly_column_names() -> List[str]:
    """The three columns of nyxhip_hexpoly_batch / _tiles, enum order."""
    return _catalogue(_abi.HEXPOLY_COLS, load().nyxhip_hexpoly_column_name, (), "hexagonality / polygonality column")


def ih_column_names() -> List[str]:
    """The 46 columns of nyxhip_ih_batch / _tiles, enum order."""
    return _catalogue(_abi.IH_COLS, load().nyxhip_ih_column_name, (), "intensity-histogram column")


def imq_column_names() -> List[str]:
    """The 4 columns of nyxhip_imq_batch / _tiles / _slides, enum order."""
    return _catalogue(_abi.IMQ_COLS, load().nyxhip_imq_column_name, (), "image-quality column")


def wsgroup_column_names(ws_mask: int) -> List[str]:
    """The columns of nyxhip_wsgroup_slides for a whole-slide group mask (_abi.WS_*): blocks in the order of the bits."""
    return _catalogue(load().nyxhip_wsgroup_n_columns, load().nyxhip_wsgroup_column_name, (ws_mask,), "whole-slide group column", "whole-slide group mask")


def vol_column_names(vmask: int, s: _abi.Settings) -> List[str]:
    """The columns of nyxhip_featurize_volumes for a volume mask (_abi.VFAM_*)."""
    return _catalogue(load().nyxhip_vol_n_columns, load().nyxhip_vol_column_name, (vmask, C.byref(s)), "volume column", "volume mask")


def voltex_column_names(tmask: int) -> List[str]:
    """The columns of nyxhip_featurize_volumes_tex for a texture mask (_abi.VTEX_*)."""
    return _catalogue(load().nyxhip_voltex_n_columns, load().nyxhip_voltex_column_name, (tmask,), "volume texture column", "volume texture mask")


def volzone_column_names(zmask: int) -> List[str]:
    """The columns of nyxhip_featurize_volumes_zones for a zone mask (_abi.VZONE_*)."""
    return _catalogue(load().nyxhip_volzone_n_columns, load().nyxhip_volzone_column_name, (zmask,), "volume zone column", "volume zone mask")


def voldzone_column_names(dmask: int = _abi.VDZ_GLDZM) -> List[str]:
    """The columns of nyxhip_featurize_volumes_dzones for a distance-zone mask (_abi.VDZ_*)."""
    return _catalogue(load().nyxhip_voldzone_n_columns, load().nyxhip_voldzone_column_name, (dmask,), "volume distance-zone column", "volume distance-zone mask")


def volshape_column_names(smask: int = _abi.VSHAPE_MORPHOLOGY) -> List[str]:
    """The columns of nyxhip_featurize_volumes_shape for a shape mask (_abi.VSHAPE_*)."""
    return _catalogue(load().nyxhip_vshape_n_columns, load().nyxhip_vshape_column_name, (smask,), "volume shape column", "volume shape mask")


def morph_column_names(mmask: int = _abi.MORPH_ALL) -> List[str]:
    """The columns of nyxhip_morph_batch / _tiles for a morphology mask (_abi.MORPH_*), enum order."""
    return _catalogue(load().nyxhip_morph_n_columns, load().nyxhip_morph_column_name, (mmask,), "morphology column", "morphology mask")


# Contexts still open at interpreter exit are destroyed here, while the HIP runtime is certainly alive (Python's atexit handlers
# run before the C library's): a context freed by the garbage collector during shutdown could reach hipFree / hipStreamDestroy
# after the runtime's own exit handlers.
_live_contexts = weakref.WeakSet()


def _close_live_contexts():
    for ctx in list(_live_contexts):
        try:
            ctx.close()
        except Exception:
            pass


atexit.register(_close_live_contexts)


class AssembledVolumes(NamedTuple):
    """What Context.assemble_volumes_* returns: the device batch (valid until the context's next assemble / release_volumes / close), its
    row count, host copies of the rows' labels and volume indices, and the device pointer of the volume indices (None: no rows)."""
    batch: _abi.Batch3D
    n_roi: int
    labels: np.ndarray
    volume_index: np.ndarray
    volume_index_ptr: Optional[int]


class Context:
    """One ``nyxhip_ctx`` bound to one GPU (one per process rank)."""

    def __init__(self, device: int = 0):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.nyxhip_init(device, C.byref(h))
        if rc != 0:
            raise NyxHipError(rc, (self._lib.nyxhip_last_error(None) or b"").decode())
        self._h = h
        self.device = device
        _live_contexts.add(self)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nyxhip_destroy(self._h)
            self._h = None

    def __del__(self):
        # a context that is still alive when the interpreter shuts down was closed by _close_live_contexts (atexit: before the
        # HIP runtime's own exit handlers); one collected later than that must not call into a runtime that may be gone
        try:
            if sys is None or sys.is_finalizing():    # (module globals may already be cleared at that point)
                return
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise NyxHipError(rc, (self._lib.nyxhip_last_error(self._h) or b"").decode())

    def set_stream(self, stream_ptr: Optional[int]):
        self._check(self._lib.nyxhip_set_stream(self._h, C.c_void_p(stream_ptr)))

    def n_columns(self, mask: int, s: _abi.Settings) -> int:
        return self._lib.nyxhip_n_columns(mask, C.byref(s))

    def featurize_host(self, batch: _abi.HostBatch, mask: int, s: _abi.Settings) -> np.ndarray:
        """Host arrays in, host table out (synchronous)."""
        ncol = self.n_columns(mask, s)
        out = np.empty((batch.n_roi, ncol), np.float64)
        cb = batch.c_struct()
        if (mask & _abi.FAM_NEEDS_ORIGIN) and batch.origin_unrepresentable:
            raise ValueError("the caliper families, the chords and the circle diameters need the ROIs' origins, and this batch's lie below 0 or beyond 32 bits")
        if batch.origin_x is not None:           # the ROIs' positions: read by the caliper families, the chords and the circle diameters
            self._check(self._lib.nyxhip_featurize_batch_at(self._h, C.byref(cb), batch.origin_x.ctypes.data, batch.origin_y.ctypes.data, mask,
                                                            C.byref(s), out.ctypes.data, ncol))
        else:
            self._check(self._lib.nyxhip_featurize_batch(self._h, C.byref(cb), mask, C.byref(s), out.ctypes.data, ncol))
        return out

    def neighbors_host(self, batch: _abi.HostBatch, distance: int, s: _abi.Settings) -> np.ndarray:
        """The neighbor columns [n_roi x 9] of a host batch (nyxhip_neighbors_batch).  batch.image_offset: the rows of every image (None:
        one image); inside an image the rows ascend in roi_label.  batch.origin_x / origin_y: the boxes' places in their image."""
        if batch.origin_unrepresentable:
            raise ValueError("the neighbor class needs the ROIs' origins, and this batch's lie below 0 or beyond 32 bits")
        out = np.empty((batch.n_roi, _abi.NEIGHBOR_COLS), np.float64)
        cb = batch.c_struct()
        io = batch.image_offset
        self._check(self._lib.nyxhip_neighbors_batch(
            self._h, C.byref(cb), batch.origin_x.ctypes.data if batch.origin_x is not None else None,
            batch.origin_y.ctypes.data if batch.origin_y is not None else None, io.ctypes.data if io is not None else None,
            len(io) - 1 if io is not None else 0, int(distance), C.byref(s), out.ctypes.data, _abi.NEIGHBOR_COLS))
        return out

    def _tiles_table(self, entry, lead: tuple, ncol: int, inten: np.ndarray, label: np.ndarray, s: _abi.Settings, max_device_bytes: int):
        """(tile_index, labels, table [n_roi x ncol]) of a stack [n_tiles, H, W] of host tiles through the tile entry of a class with entries of
        its own: entry(ctx, tiles, *lead, settings, outputs...) keeps its rows in the context, nyxhip_fetch_result copies them out."""
        if inten.shape != label.shape or inten.ndim != 3:
            raise ValueError("stacks must be 3-D arrays [n_tiles, H, W] of the same shape")
        dt = {np.dtype(np.uint8): _abi.U8, np.dtype(np.uint16): _abi.U16, np.dtype(np.uint32): _abi.U32}
        inten = np.ascontiguousarray(inten if inten.dtype in dt else inten.astype(np.uint32))
        label = np.ascontiguousarray(label if label.dtype in dt else label.astype(np.uint32))
        nt, h, w = inten.shape
        if nt == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, ncol))
        t = _abi.Tiles()
        t.inten = inten.ctypes.data; t.label = label.ctypes.data
        t.inten_dtype = dt[inten.dtype]; t.label_dtype = dt[label.dtype]
        t.width = w; t.height = h; t.n_tiles = nt; t.memory = _abi.MEM_HOST; t.slide_mode = _abi.SLIDE_MONTAGE
        t.max_device_bytes = int(max_device_bytes)
        n = C.c_uint64(0)
        self._check(entry(self._h, C.byref(t), *lead, C.byref(s), None, None, 0, None, 0, C.byref(n)))
        labels = np.zeros(n.value, np.uint32); tiles = np.zeros(n.value, np.uint32); table = np.empty((n.value, ncol), np.float64)
        self._check(self._lib.nyxhip_fetch_result(self._h, labels.ctypes.data, tiles.ctypes.data, table.ctypes.data, ncol))
        return tiles, labels, table

    def neighbors_tiles_host(self, inten: np.ndarray, label: np.ndarray, distance: int, s: _abi.Settings, max_device_bytes: int = 0):
        """The neighbor columns of a stack [n_tiles, H, W] of host tiles, one image per tile (nyxhip_neighbors_tiles).  Returns
        (tile_index, labels, table [n_roi x 9]) in the (tile, label) row order of featurize_tiles_host."""
        return self._tiles_table(self._lib.nyxhip_neighbors_tiles, (int(distance),), _abi.NEIGHBOR_COLS, inten, label, s, max_device_bytes)

    def hexpoly_host(self, batch: _abi.HostBatch, distance: int, s: _abi.Settings) -> np.ndarray:
        """POLYGONALITY_AVE, HEXAGONALITY_AVE, HEXAGONALITY_STDDEV [n_roi x 3] of a host batch (nyxhip_hexpoly_batch); -1, NaN and inf are
        left in place.  batch.image_offset, the label order and the origins as in neighbors_host."""
        if batch.origin_unrepresentable:
            raise ValueError("the hexagonality / polygonality class needs the ROIs' origins, and this batch's lie below 0 or beyond 32 bits")
        out = np.empty((batch.n_roi, _abi.HEXPOLY_COLS), np.float64)
        cb = batch.c_struct()
        io = batch.image_offset
        self._check(self._lib.nyxhip_hexpoly_batch(
            self._h, C.byref(cb), batch.origin_x.ctypes.data if batch.origin_x is not None else None,
            batch.origin_y.ctypes.data if batch.origin_y is not None else None, io.ctypes.data if io is not None else None,
            len(io) - 1 if io is not None else 0, int(distance), C.byref(s), out.ctypes.data, _abi.HEXPOLY_COLS))
        return out

    def hexpoly_device(self, cb: _abi.Batch, origin_x_ptr: Optional[int], origin_y_ptr: Optional[int], image_offset_ptr: Optional[int], n_images: int,
                       distance: int, s: _abi.Settings, out_ptr: int, ld: int):
        """Device pointers in ``cb`` (roi_label, px_offset, x, y, inten, bbox_w, bbox_h), device origins and image offsets (or None) and a
        device table; synchronous (nyxhip_hexpoly_batch)."""
        self._check(self._lib.nyxhip_hexpoly_batch(self._h, C.byref(cb), C.c_void_p(origin_x_ptr), C.c_void_p(origin_y_ptr), C.c_void_p(image_offset_ptr),
                                                   int(n_images), int(distance), C.byref(s), C.c_void_p(out_ptr), ld))

    def hexpoly_tiles_host(self, inten: np.ndarray, label: np.ndarray, distance: int, s: _abi.Settings, max_device_bytes: int = 0):
        """The three columns of a stack [n_tiles, H, W] of host tiles, one image per tile (nyxhip_hexpoly_tiles).  Returns (tile_index, labels,
        table [n_roi x 3]) in the (tile, label) row order of featurize_tiles_host."""
        return self._tiles_table(self._lib.nyxhip_hexpoly_tiles, (int(distance),), _abi.HEXPOLY_COLS, inten, label, s, max_device_bytes)

    def morph_host(self, batch: _abi.HostBatch, mmask: int, s: _abi.Settings) -> np.ndarray:
        """The columns of morphology mask `mmask` (_abi.MORPH_*) of a host batch (nyxhip_morph_batch); NaN / inf are left in place.
        batch.origin_x / origin_y: the boxes' places in their image (None: (0, 0))."""
        ncol = self._lib.nyxhip_morph_n_columns(mmask)
        if ncol < 0:
            raise NyxHipError(1, f"bad morphology mask {mmask:#x}")
        if batch.origin_unrepresentable:
            raise ValueError("the morphology classes need the ROIs' origins, and this batch's lie below 0 or beyond 32 bits")
        out = np.empty((batch.n_roi, ncol), np.float64)
        cb = batch.c_struct()
        self._check(self._lib.nyxhip_morph_batch(
            self._h, C.byref(cb), batch.origin_x.ctypes.data if batch.origin_x is not None else None,
            batch.origin_y.ctypes.data if batch.origin_y is not None else None, mmask, C.byref(s), out.ctypes.data, ncol))
        return out

    def morph_device(self, cb: _abi.Batch, origin_x_ptr: Optional[int], origin_y_ptr: Optional[int], mmask: int, s: _abi.Settings, out_ptr: int, ld: int):
        """Device pointers in ``cb`` (px_offset, x, y, inten, bbox_w, bbox_h), device origins (or None) and a device table; synchronous
        (nyxhip_morph_batch)."""
        self._check(self._lib.nyxhip_morph_batch(self._h, C.byref(cb), C.c_void_p(origin_x_ptr), C.c_void_p(origin_y_ptr), mmask, C.byref(s),
                                                 C.c_void_p(out_ptr), ld))

    def morph_tiles_host(self, inten: np.ndarray, label: np.ndarray, mmask: int, s: _abi.Settings, max_device_bytes: int = 0):
        """The columns of morphology mask `mmask` of a stack [n_tiles, H, W] of host tiles, one image per tile (nyxhip_morph_tiles).
        Returns (tile_index, labels, table) in the (tile, label) row order of featurize_tiles_host."""
        if inten.shape != label.shape or inten.ndim != 3:
            raise ValueError("stacks must be 3-D arrays [n_tiles, H, W] of the same shape")
        ncol = self._lib.nyxhip_morph_n_columns(mmask)
        if ncol < 0:
            raise NyxHipError(1, f"bad morphology mask {mmask:#x}")
        return self._tiles_table(self._lib.nyxhip_morph_tiles, (mmask,), ncol, inten, label, s, max_device_bytes)

    def ih_host(self, batch: _abi.HostBatch, s: _abi.Settings) -> np.ndarray:
        """The intensity-histogram columns [n_roi x 46] of a host batch (nyxhip_ih_batch); NaN / inf are left in place."""
        out = np.empty((batch.n_roi, _abi.IH_COLS), np.float64)
        cb = batch.c_struct()
        self._check(self._lib.nyxhip_ih_batch(self._h, C.byref(cb), C.byref(s), out.ctypes.data, _abi.IH_COLS))
        return out

    def ih_device(self, cb: _abi.Batch, s: _abi.Settings, out_ptr: int, ld: int):
        """Device pointers in ``cb`` (px_offset, inten, min_inten, max_inten) and a device table; synchronous (nyxhip_ih_batch)."""
        self._check(self._lib.nyxhip_ih_batch(self._h, C.byref(cb), C.byref(s), C.c_void_p(out_ptr), ld))

    def ih_tiles_host(self, inten: np.ndarray, label: np.ndarray, s: _abi.Settings, max_device_bytes: int = 0):
        """The intensity-histogram columns of a stack [n_tiles, H, W] of host tiles (nyxhip_ih_tiles).  Returns (tile_index, labels,
        table [n_roi x 46]) in the (tile, label) row order of featurize_tiles_host."""
        return self._tiles_table(self._lib.nyxhip_ih_tiles, (), _abi.IH_COLS, inten, label, s, max_device_bytes)

    def _volume_table(self, entry, n_columns, mask_noun: str, batch: _abi.HostBatch3D, mask: int, n_lead: tuple, lead: tuple, stated: bool,
                      max_device_bytes: int) -> np.ndarray:
        """The table [n_roi x n_columns(mask, *n_lead)] of a host batch through a volume entry: entry(ctx, batch, mask, *lead, table, ld)."""
        ncol = n_columns(mask, *n_lead)
        if ncol < 0:
            raise NyxHipError(1, f"bad {mask_noun} {mask:#x}")
        out = np.empty((batch.n_roi, ncol), np.float64)
        cb = batch.c_struct(stated=stated, max_device_bytes=max_device_bytes)
        self._check(entry(self._h, C.byref(cb), mask, *lead, out.ctypes.data, ncol))
        return out

    def volumes_host(self, batch: _abi.HostBatch3D, vmask: int, s: _abi.Settings, stated: bool = False, max_device_bytes: int = 0) -> np.ndarray:
        """The volume table [n_roi x nyxhip_vol_n_columns] of a host batch (nyxhip_featurize_volumes); NaN / inf are left in place."""
        return self._volume_table(self._lib.nyxhip_featurize_volumes, self._lib.nyxhip_vol_n_columns, "volume mask", batch, vmask, (C.byref(s),), (C.byref(s),), stated,
                                  max_device_bytes)

    def volumes_device(self, cb: _abi.Batch3D, vmask: int, s: _abi.Settings, out_ptr: int, ld: int):
        """Device pointers in ``cb`` and a device table; synchronous (nyxhip_featurize_volumes)."""
        self._check(self._lib.nyxhip_featurize_volumes(self._h, C.byref(cb), vmask, C.byref(s), C.c_void_p(out_ptr), ld))

    def volumes_tex_host(self, batch: _abi.HostBatch3D, tmask: int, s: _abi.Settings, t: _abi.VolTexSettings, stated: bool = False,
                         max_device_bytes: int = 0) -> np.ndarray:
        """The texture table [n_roi x nyxhip_voltex_n_columns] of a host batch (nyxhip_featurize_volumes_tex); NaN / inf are left in place."""
        return self._volume_table(self._lib.nyxhip_featurize_volumes_tex, self._lib.nyxhip_voltex_n_columns, "volume texture mask", batch, tmask, (),
                                  (C.byref(s), C.byref(t)), stated, max_device_bytes)

    def volumes_tex_device(self, cb: _abi.Batch3D, tmask: int, s: _abi.Settings, t: _abi.VolTexSettings, out_ptr: int, ld: int):
        """Device pointers in ``cb`` and a device table; synchronous (nyxhip_featurize_volumes_tex)."""
        self._check(self._lib.nyxhip_featurize_volumes_tex(self._h, C.byref(cb), tmask, C.byref(s), C.byref(t), C.c_void_p(out_ptr), ld))

    def volumes_zones_host(self, batch: _abi.HostBatch3D, zmask: int, s: _abi.Settings, t: _abi.VolZoneSettings, stated: bool = False,
                           max_device_bytes: int = 0) -> np.ndarray:
        """The zone table [n_roi x nyxhip_volzone_n_columns] of a host batch (nyxhip_featurize_volumes_zones); NaN / inf are left in place."""
        return self._volume_table(self._lib.nyxhip_featurize_volumes_zones, self._lib.nyxhip_volzone_n_columns, "volume zone mask", batch, zmask, (),
                                  (C.byref(s), C.byref(t)), stated, max_device_bytes)

    def volumes_zones_device(self, cb: _abi.Batch3D, zmask: int, s: _abi.Settings, t: _abi.VolZoneSettings, out_ptr: int, ld: int):
        """Device pointers in ``cb`` and a device table; synchronous (nyxhip_featurize_volumes_zones)."""
        self._check(self._lib.nyxhip_featurize_volumes_zones(self._h, C.byref(cb), zmask, C.byref(s), C.byref(t), C.c_void_p(out_ptr), ld))

    def volumes_dzones_host(self, batch: _abi.HostBatch3D, dmask: int, s: _abi.Settings, stated: bool = False, max_device_bytes: int = 0) -> np.ndarray:
        """The distance-zone table [n_roi x 18] of a host batch (nyxhip_featurize_volumes_dzones); NaN / inf are left in place."""
        return self._volume_table(self._lib.nyxhip_featurize_volumes_dzones, self._lib.nyxhip_voldzone_n_columns, "volume distance-zone mask", batch, dmask, (),
                                  (C.byref(s),), stated, max_device_bytes)

    def volumes_dzones_device(self, cb: _abi.Batch3D, dmask: int, s: _abi.Settings, out_ptr: int, ld: int):
        """Device pointers in ``cb`` and a device table; synchronous (nyxhip_featurize_volumes_dzones)."""
        self._check(self._lib.nyxhip_featurize_volumes_dzones(self._h, C.byref(cb), dmask, C.byref(s), C.c_void_p(out_ptr), ld))

    def volumes_shape_host(self, batch: _abi.HostBatch3D, smask: int, s: _abi.Settings, stated: bool = False, max_device_bytes: int = 0) -> np.ndarray:
        """The shape table [n_roi x 14] of a host batch (nyxhip_featurize_volumes_shape); NaN / inf are left in place."""
        return self._volume_table(self._lib.nyxhip_featurize_volumes_shape, self._lib.nyxhip_vshape_n_columns, "volume shape mask", batch, smask, (),
                                  (C.byref(s),), stated, max_device_bytes)

    def volumes_shape_device(self, cb: _abi.Batch3D, smask: int, s: _abi.Settings, out_ptr: int, ld: int):
        """Device pointers in ``cb`` and a device table; synchronous (nyxhip_featurize_volumes_shape)."""
        self._check(self._lib.nyxhip_featurize_volumes_shape(self._h, C.byref(cb), smask, C.byref(s), C.c_void_p(out_ptr), ld))

    def _assembled(self, vols: _abi.Volumes) -> "AssembledVolumes":
        cb, vi = _abi.Batch3D(), C.c_void_p()
        self._check(self._lib.nyxhip_assemble_volumes(self._h, C.byref(vols), C.byref(cb), C.byref(vi)))
        n = int(cb.n_roi)
        labels, vol = np.empty(n, np.uint32), np.empty(n, np.uint32)
        self._check(self._lib.nyxhip_assembled_rows(self._h, labels.ctypes.data, vol.ctypes.data, n))
        return AssembledVolumes(cb, n, labels, vol, vi.value)

    def assemble_volumes_host(self, inten: np.ndarray, label: np.ndarray, max_device_bytes: int = 0) -> "AssembledVolumes":
        """The ROIs of host volumes [n, z, y, x] (uint8 / uint16 / uint32 each) as a device batch the context owns until the next
        assemble, release_volumes() or close() (nyxhip_assemble_volumes): rows in (volume, label) order."""
        if inten.ndim != 4 or inten.shape != label.shape:
            raise ValueError("inten and label must be [n, z, y, x] arrays of one shape")
        inten, label = np.ascontiguousarray(inten), np.ascontiguousarray(label)
        return self._assembled(_abi.volumes_struct(inten.ctypes.data, _abi.volume_dtype(inten.dtype), label.ctypes.data, _abi.volume_dtype(label.dtype),
                                                   inten.shape, _abi.MEM_HOST, max_device_bytes))

    def assemble_volumes_device(self, inten_ptr: int, inten_dtype: int, label_ptr: int, label_dtype: int, shape, max_device_bytes: int = 0) -> "AssembledVolumes":
        """As assemble_volumes_host for volumes that lie in device memory: the pointers and element types (U8 / U16 / U32) of two contiguous
        [n, z, y, x] arrays, for example torch tensors' data_ptr()."""
        return self._assembled(_abi.volumes_struct(inten_ptr, inten_dtype, label_ptr, label_dtype, shape, _abi.MEM_DEVICE, max_device_bytes))

    def release_volumes(self):
        """Frees the assembled batch and the workspaces of the scan (nyxhip_release_volumes)."""
        self._check(self._lib.nyxhip_release_volumes(self._h))

    def imq_host(self, batch: _abi.HostBatch, s: _abi.Settings) -> np.ndarray:
        """The image-quality columns [n_roi x 4] of a host batch (nyxhip_imq_batch); NaN / inf are left in place."""
        out = np.empty((batch.n_roi, _abi.IMQ_COLS), np.float64)
        cb = batch.c_struct()
        self._check(self._lib.nyxhip_imq_batch(self._h, C.byref(cb), C.byref(s), out.ctypes.data, _abi.IMQ_COLS))
        return out

    def imq_device(self, cb: _abi.Batch, s: _abi.Settings, out_ptr: int, ld: int):
        """Device pointers in ``cb`` (px_offset, x, y, inten, bbox_w, bbox_h, min_inten, max_inten) and a device table; synchronous
        (nyxhip_imq_batch)."""
        self._check(self._lib.nyxhip_imq_batch(self._h, C.byref(cb), C.byref(s), C.c_void_p(out_ptr), ld))

    def imq_tiles_host(self, inten: np.ndarray, label: np.ndarray, s: _abi.Settings, max_device_bytes: int = 0):
        """The image-quality columns of a stack [n_tiles, H, W] of host tiles (nyxhip_imq_tiles).  Returns (tile_index, labels,
        table [n_roi x 4]) in the (tile, label) row order of featurize_tiles_host."""
        return self._tiles_table(self._lib.nyxhip_imq_tiles, (), _abi.IMQ_COLS, inten, label, s, max_device_bytes)

    def imq_slides_host(self, inten: np.ndarray, s: _abi.Settings, max_device_bytes: int = 0) -> np.ndarray:
        """Whole-slide mode (nyxhip_imq_slides): a stack [n, H, W] of uint8 / uint16 / uint32 host slides, every slide one ROI that
        covers the whole image.  Returns the table [n, 4], rows in input order; NaN / inf are left in place."""
        dt = {np.dtype(np.uint8): _abi.U8, np.dtype(np.uint16): _abi.U16, np.dtype(np.uint32): _abi.U32}
        if inten.ndim != 3 or inten.dtype not in dt:
            raise ValueError("slides must be a 3-D array [n, H, W] of uint8, uint16 or uint32")
        inten = np.ascontiguousarray(inten)
        n, h, w = inten.shape
        out = np.empty((n, _abi.IMQ_COLS), np.float64)
        t = _abi.Tiles()
        t.inten = inten.ctypes.data; t.label = None
        t.inten_dtype = dt[inten.dtype]; t.width = w; t.height = h; t.n_tiles = n; t.memory = _abi.MEM_HOST
        t.max_device_bytes = int(max_device_bytes)
        self._check(self._lib.nyxhip_imq_slides(self._h, C.byref(t), C.byref(s), out.ctypes.data, _abi.IMQ_COLS))
        return out

    def imq_slides_device(self, inten_ptr: int, dtype: int, n: int, h: int, w: int, s: _abi.Settings, out_ptr: int, ld: int, max_device_bytes: int = 0):
        """The same entry on device memory: `inten_ptr` is a device array [n, h, w] of element type `dtype` (_abi.U8 / U16 / U32),
        `out_ptr` a device table [n x ld] of doubles.  Synchronous."""
        t = _abi.Tiles()
        t.inten = inten_ptr; t.label = None
        t.inten_dtype = dtype; t.width = w; t.height = h; t.n_tiles = n; t.memory = _abi.MEM_DEVICE
        t.max_device_bytes = int(max_device_bytes)
        self._check(self._lib.nyxhip_imq_slides(self._h, C.byref(t), C.byref(s), C.c_void_p(out_ptr), ld))

    def wsgroup_slides_host(self, inten: np.ndarray, ws_mask: int, s: _abi.Settings, max_device_bytes: int = 0) -> np.ndarray:
        """Whole-slide mode of the contour, moment and radial classes (nyxhip_wsgroup_slides): a stack [n, H, W] of uint8 / uint16 /
        uint32 host slides, every slide one ROI whose contour is its four corners.  Returns the table [n, nyxhip_wsgroup_n_columns],
        rows in input order; NaN / inf are left in place."""
        dt = {np.dtype(np.uint8): _abi.U8, np.dtype(np.uint16): _abi.U16, np.dtype(np.uint32): _abi.U32}
        if inten.ndim != 3 or inten.dtype not in dt:
            raise ValueError("slides must be a 3-D array [n, H, W] of uint8, uint16 or uint32")
        inten = np.ascontiguousarray(inten)
        n, h, w = inten.shape
        ncol = self._lib.nyxhip_wsgroup_n_columns(ws_mask)
        out = np.empty((n, max(ncol, 0)), np.float64)
        t = _abi.Tiles()
        t.inten = inten.ctypes.data; t.label = None
        t.inten_dtype = dt[inten.dtype]; t.width = w; t.height = h; t.n_tiles = n; t.memory = _abi.MEM_HOST
        t.max_device_bytes = int(max_device_bytes)
        self._check(self._lib.nyxhip_wsgroup_slides(self._h, C.byref(t), ws_mask, C.byref(s), out.ctypes.data, max(ncol, 1)))
        return out

    def wsgroup_slides_device(self, inten_ptr: int, dtype: int, n: int, h: int, w: int, ws_mask: int, s: _abi.Settings, out_ptr: int, ld: int,
                              max_device_bytes: int = 0):
        """The same entry on device memory: `inten_ptr` is a device array [n, h, w] of element type `dtype` (_abi.U8 / U16 / U32),
        `out_ptr` a device table [n x ld] of doubles.  Synchronous."""
        t = _abi.Tiles()
        t.inten = inten_ptr; t.label = None
        t.inten_dtype = dtype; t.width = w; t.height = h; t.n_tiles = n; t.memory = _abi.MEM_DEVICE
        t.max_device_bytes = int(max_device_bytes)
        self._check(self._lib.nyxhip_wsgroup_slides(self._h, C.byref(t), ws_mask, C.byref(s), C.c_void_p(out_ptr), ld))

    def featurize_device_async(self, cb: _abi.Batch, mask: int, s: _abi.Settings, out_ptr: int, ld: int, origin_x_ptr: Optional[int] = None,
                               origin_y_ptr: Optional[int] = None):
        """Device pointers in ``cb``; enqueues the kernel on the context's stream.  origin_*_ptr: device arrays [n_roi] of the
        ROIs' box origins (nyxhip_featurize_batch_async_at)."""
        if origin_x_ptr is not None:
            self._check(self._lib.nyxhip_featurize_batch_async_at(self._h, C.byref(cb), C.c_void_p(origin_x_ptr), C.c_void_p(origin_y_ptr), mask,
                                                                  C.byref(s), C.c_void_p(out_ptr), ld))
        else:
            self._check(self._lib.nyxhip_featurize_batch_async(self._h, C.byref(cb), mask, C.byref(s), C.c_void_p(out_ptr), ld))

    def featurize_tile_host(self, inten: np.ndarray, label: np.ndarray, mask: int, s: _abi.Settings, max_label: Optional[int] = None):
        """One intensity / label tile pair (host arrays) through the fused device path: label scan + ROI assembly + reduce.
        Returns (labels ascending, table).  `max_label` (v1 semantics): a label above it is an error."""
        if inten.shape != label.shape or inten.ndim != 2:
            raise ValueError("tiles must be 2-D arrays of the same shape")
        if max_label is not None:
            inten = np.ascontiguousarray(inten, np.uint32)
            label = np.ascontiguousarray(label, np.uint32)
            ncol = self.n_columns(mask, s)
            cap = max(1, min(max_label, inten.size))
            labels = np.zeros(cap, np.uint32)
            table = np.empty((cap, ncol), np.float64)
            n = C.c_uint64(0)
            self._check(self._lib.nyxhip_featurize_tile(self._h, inten.ctypes.data, label.ctypes.data, inten.shape[1], inten.shape[0],
                                                        _abi.MEM_HOST, max_label, mask, C.byref(s), labels.ctypes.data, cap,
                                                        table.ctypes.data, ncol, C.byref(n)))
            return labels[: n.value], table[: n.value]
        _, labels, table = self.featurize_tiles_host(inten[None], label[None], mask, s)
        return labels, table

    def featurize_tiles_host(self, inten: np.ndarray, label: np.ndarray, mask: int, s: _abi.Settings, slide_mode: int = _abi.SLIDE_MONTAGE,
                             slide_min=None, slide_max=None, max_device_bytes: int = 0, contexts: Optional[list] = None, own_mapping: bool = False):
        """A stack [n_tiles, H, W] of host tiles through the fused device path (nyxhip_featurize_tiles_v2).  uint8 / uint16 /
        uint32 arrays are handed over as they are (the kernels widen); anything else is cast to uint32 first.  Label values are
        arbitrary.  Returns (tile_index, labels, table) with rows ordered by (tile, label), sized by the ROI count the device
        scan found.  `contexts`: more contexts (one per GPU) -> nyxhip_featurize_tiles_sharded block-partitions the stack.
        `own_mapping`: the caller's statement that both stacks are mappings of their own (e.g. numpy arrays over an mmap): they
        are registered for DMA in place (NYXHIP_MEM_HOST_OWN_MAPPING); otherwise the bytes pass through the library's pinned
        staging ring, which assumes nothing about the allocator."""
        if inten.shape != label.shape or inten.ndim != 3:
            raise ValueError("stacks must be 3-D arrays [n_tiles, H, W] of the same shape")
        dt = {np.dtype(np.uint8): _abi.U8, np.dtype(np.uint16): _abi.U16, np.dtype(np.uint32): _abi.U32}
        inten = np.ascontiguousarray(inten if inten.dtype in dt else inten.astype(np.uint32))
        label = np.ascontiguousarray(label if label.dtype in dt else label.astype(np.uint32))
        ncol = self.n_columns(mask, s)
        nt, h, w = inten.shape
        t = _abi.Tiles()
        t.inten = inten.ctypes.data; t.label = label.ctypes.data
        t.inten_dtype = dt[inten.dtype]; t.label_dtype = dt[label.dtype]
        t.width = w; t.height = h; t.n_tiles = nt; t.memory = _abi.MEM_HOST_OWN_MAPPING if own_mapping else _abi.MEM_HOST; t.slide_mode = slide_mode
        keep = []
        if slide_mode == _abi.SLIDE_GIVEN:
            keep = [np.ascontiguousarray(slide_min, np.float64), np.ascontiguousarray(slide_max, np.float64)]
            if keep[0].shape != (nt,) or keep[1].shape != (nt,):
                raise ValueError("slide_min / slide_max must hold one value per tile")
            t.slide_min = keep[0].ctypes.data; t.slide_max = keep[1].ctypes.data
        t.max_device_bytes = int(max_device_bytes)
        n = C.c_uint64(0)
        if nt == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, ncol))
        ctxs = [self] + [c for c in (contexts or []) if c is not self]
        if len(ctxs) > 1:
            arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
            self._check(self._lib.nyxhip_featurize_tiles_sharded(arr, len(ctxs), C.byref(t), mask, C.byref(s), None, None, 0, None, 0, C.byref(n)))
            labels = np.zeros(n.value, np.uint32); tiles = np.zeros(n.value, np.uint32); table = np.empty((n.value, ncol), np.float64)
            self._check(self._lib.nyxhip_fetch_result_sharded(arr, len(ctxs), labels.ctypes.data, tiles.ctypes.data, table.ctypes.data, ncol))
            return tiles, labels, table
        self._check(self._lib.nyxhip_featurize_tiles_v2(self._h, C.byref(t), mask, C.byref(s), None, None, 0, None, 0, C.byref(n)))
        labels = np.zeros(n.value, np.uint32)
        tiles = np.zeros(n.value, np.uint32)
        table = np.empty((n.value, ncol), np.float64)
        self._check(self._lib.nyxhip_fetch_result(self._h, labels.ctypes.data, tiles.ctypes.data, table.ctypes.data, ncol))
        return tiles, labels, table

    def featurize_slides_host(self, inten: np.ndarray, mask: int, s: _abi.Settings, max_device_bytes: int = 0) -> np.ndarray:
        """Whole-slide mode (nyxhip_featurize_slides): a stack [n, H, W] of uint8 / uint16 / uint32 host slides, every slide one ROI
        with label 1 that covers the whole image.  Returns the table [n, n_columns], rows in input order; NaN / inf are left in place."""
        dt = {np.dtype(np.uint8): _abi.U8, np.dtype(np.uint16): _abi.U16, np.dtype(np.uint32): _abi.U32}
        if inten.ndim != 3 or inten.dtype not in dt:
            raise ValueError("slides must be a 3-D array [n, H, W] of uint8, uint16 or uint32")
        inten = np.ascontiguousarray(inten)
        n, h, w = inten.shape
        ncol = self.n_columns(mask, s)
        out = np.empty((n, max(ncol, 0)), np.float64)
        t = _abi.Tiles()
        t.inten = inten.ctypes.data; t.label = None
        t.inten_dtype = dt[inten.dtype]; t.width = w; t.height = h; t.n_tiles = n; t.memory = _abi.MEM_HOST
        t.max_device_bytes = int(max_device_bytes)
        self._check(self._lib.nyxhip_featurize_slides(self._h, C.byref(t), mask, C.byref(s), out.ctypes.data, max(ncol, 1)))
        return out

    def featurize_slides_device(self, inten_ptr: int, dtype: int, n: int, h: int, w: int, mask: int, s: _abi.Settings, out_ptr: int, ld: int,
                                max_device_bytes: int = 0):
        """The same entry on device memory: `inten_ptr` is a device array [n, h, w] of element type `dtype` (_abi.U8 / U16 / U32),
        `out_ptr` a device table [n x ld] of doubles.  Synchronous."""
        t = _abi.Tiles()
        t.inten = inten_ptr; t.label = None
        t.inten_dtype = dtype; t.width = w; t.height = h; t.n_tiles = n; t.memory = _abi.MEM_DEVICE
        t.max_device_bytes = int(max_device_bytes)
        self._check(self._lib.nyxhip_featurize_slides(self._h, C.byref(t), mask, C.byref(s), C.c_void_p(out_ptr), ld))

    def sync(self):
        self._check(self._lib.nyxhip_sync(self._h))

    def timing(self, on: bool, groups: bool = False):
        """on: two events around every call (timing_get); groups: also around every launch group (the "ms" of launch_report)."""
        self._check(self._lib.nyxhip_timing_enable(self._h, (2 if groups else 1) if on else 0))
        self._check(self._lib.nyxhip_timing_reset(self._h))

    def timing_reset(self):
        self._check(self._lib.nyxhip_timing_reset(self._h))

    def roi_words(self, n_roi: int):
        """(matrix orders stated, closing flags pending) among the first n_roi entries of the per-call tables as the last call left
        them; waits for the stream (nyxhip_debug_roi_words)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.nyxhip_debug_roi_words(self._h, n_roi, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def launch_report(self):
        """The size classes of the last featurize_batch call as launched (list of dicts; nyxhip_launch_report)."""
        import json
        buf = C.create_string_buffer(1 << 14)
        n = self._lib.nyxhip_launch_report(self._h, buf, len(buf))
        if n < 0:
            raise NyxHipError(-n, "launch report")
        return json.loads(buf.value.decode())

    def timing_get(self):
        ms = C.c_double()
        n = C.c_uint64()
        self._check(self._lib.nyxhip_timing_get(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value
