"""`ImageQuality` -- the reference's second 2-D Python class (src/nyx/python/nyxus/nyxus.py:1491 of the reference), served by the image-quality
entries of include/nyxhip.h: nyxhip_imq_tiles for labelled images, nyxhip_imq_slides for whole images.

Four of the six `FeatureIMQ` codes are served (featureset.h:920-931 of the reference): FOCUS_SCORE, LOCAL_FOCUS_SCORE, MAX_SATURATION,
MIN_SATURATION.  The codes live in an enum of their own and arrive through a class of their own, so their expansion lives here:
`featureset.expand`, its groups and order lists, and the `Nyxus` class know nothing of them.

The workflows -- argument checks, 2-D -> 3-D promotion, names, the negative-intensity shift, file stacks, the DataFrame layout -- are
`Nyxus`'s own methods; this class only answers the questions they ask: which columns, and which entry produces the table.
"""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np

from . import _lib
from .nyxus import Nyxus

# enum order (FeatureIMQ)
IMQ_FEATURES = ["FOCUS_SCORE", "LOCAL_FOCUS_SCORE", "MAX_SATURATION", "MIN_SATURATION"]
IMQ_GROUP = "*ALL_IMQ*"
# the two codes of FeatureIMQ that are not served, and why (include/nyxhip.h)
IMQ_UNSERVED = {
    "POWER_SPECTRUM_SLOPE": "the reference bins every FFT output by floor(sqrt(value)) + 1 -- the value, not its radius -- and indexes a table of "
                            "max(rows, cols) radii with indices up to the padded size (power_spectrum.cpp:85-90, :168-175): a discontinuous "
                            "function of floating-point FFT outputs with an out-of-bounds read, which no tolerance can pin",
    "SHARPNESS": "the reference 'transposes back' with a sequential in-place swap loop (sharpness.cpp:200-205) that is the identity for a "
                 "square box and a shape-dependent scramble for any other, w * h dependent steps per ROI, and vets the value against nothing",
}

_VALID_KEYS = {"neighbor_distance", "pixels_per_micron", "coarse_gray_depth", "n_feature_calc_threads", "ibsi", "gabor_kersize", "gabor_gamma",
               "gabor_sig2lam", "gabor_f0", "channel_signature", "min_intensity", "max_intensity", "ram_limit", "verbose", "anisotropy_x",
               "anisotropy_y", "use_gpu_device"}


def expand_imq(features: List[str]) -> List[str]:
    """The requested FeatureIMQ codes in enum order.  `*ALL_IMQ*` (any letter case) gives the four served codes; the two unserved codes
    raise ValueError with the reason; any other name raises ValueError pointing to `Nyxus`."""
    want = set()
    for f in features:
        if not isinstance(f, str):
            raise ValueError(f"feature names must be strings, got {f!r}")
        u = f.strip().upper()
        if u == IMQ_GROUP:
            want.update(IMQ_FEATURES)
        elif u in IMQ_FEATURES:
            want.add(u)
        elif u in IMQ_UNSERVED:
            raise ValueError(f"image-quality feature {u} is not served: {IMQ_UNSERVED[u]}")
        else:
            raise ValueError(f"'{f}' is not an image-quality feature: ImageQuality serves {IMQ_FEATURES} and {IMQ_GROUP}; "
                             "every other 2-D feature belongs to the Nyxus class")
    if not want:
        raise ValueError("no features requested")
    return [c for c in IMQ_FEATURES if c in want]


class _SlideEntry:
    """What `Nyxus._featurize_slides` asks of a context, answered by nyxhip_imq_slides."""

    def __init__(self, ctx: _lib.Context):
        self._ctx = ctx

    def featurize_slides_host(self, inten: np.ndarray, mask: int, s, max_device_bytes: int = 0) -> np.ndarray:
        return self._ctx.imq_slides_host(inten, s, max_device_bytes=max_device_bytes)


class ImageQuality(Nyxus):
    def __init__(self, features: List[str], **kwargs):
        invalid = set(kwargs) - _VALID_KEYS
        if invalid:
            print(f"Warning: unexpected keyword argument(s): {', '.join(invalid)}")
        if kwargs.get("coarse_gray_depth", 256) <= 0:
            raise ValueError("Custom number of grayscale levels (parameter coarse_gray_depth, default=256) must be non-negative.")
        kw = {k: v for k, v in kwargs.items() if k in _VALID_KEYS}
        kw.setdefault("coarse_gray_depth", 256)
        super().__init__(features, **kw)       # the remaining checks are word for word the reference's for both classes

    def _set_features(self, features: List[str]):
        self._features = list(features)
        self._requested = expand_imq(self._features)
        self._mask, self._neighbors, self._ih = 0, False, False

    def _columns(self):
        names = _lib.imq_column_names()
        sel = [names.index(c) for c in self._requested]
        return [names[i] for i in sel], sel

    def _featurize_stack(self, I: np.ndarray, M: np.ndarray, slide_mode: int):
        tiles, labels, table = self._context().imq_tiles_host(I, M, self._settings, max_device_bytes=self._device_budget())
        _lib.load().nyxhip_finalize_table(table.ctypes.data, table.shape[0], table.shape[1], table.shape[1], C.c_double(self._settings.soft_nan))
        return tiles, labels, table

    def _whole_slide_refusals(self):
        """Every served code exists in whole-slide mode."""

    def _featurize_slides(self, intensity_files: list):
        real = self._context
        self._context = lambda: _SlideEntry(real())
        try:
            return super()._featurize_slides(intensity_files)
        finally:
            del self._context
