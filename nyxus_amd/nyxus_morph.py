"""nyxus_amd.NyxusMorphology -- class `Nyxus` plus the 41 codes of the 2-D morphology entries (featureset_morph): basic morphology,
contour, convex hull and extrema.  `Nyxus` itself keeps refusing them (every bit of its family mask is spoken for); this class serves
them through nyxhip_morph_tiles and puts their table to the right of the others, the way the neighbor and intensity-histogram tables
are placed.  Columns are selected by name, in enum order."""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np

from . import _lib, featureset, featureset_morph
from .nyxus import Nyxus


class NyxusMorphology(Nyxus):
    def _set_features(self, features: List[str]):
        """self._morph: the morphology mask (_abi.MORPH_*) of the requested codes; everything else as in Nyxus._set_features (a request
        of morphology codes alone leaves the family mask 0: no family call)."""
        self._features = list(features)
        full, self._morph, self._requested = featureset_morph.expand_morph(self._features)
        self._mask, self._neighbors = featureset.split_neighbors(full)
        self._ih = featureset.split_ih(full)

    def _active(self):
        """As Nyxus._active; the morphology codes do not depend on `ibsi`."""
        ih = self._ih and bool(self._settings.ibsi)
        req = self._requested
        if self._ih and not ih:
            req = [c for c in req if featureset.FAMILY_OF.get(c) != featureset.FAM_IH]
        if not req:
            raise ValueError("no features requested")
        return req, ih

    def _featurize_stack(self, I: np.ndarray, M: np.ndarray, slide_mode: int):
        """The tables of Nyxus._featurize_stack and, to their right, the morphology table of the stack (one image per tile: the origins
        are the boxes' places in their image).  The morphology call runs on the first context only."""
        _, ih = self._active()
        tiles = labels = table = None
        if self._mask or self._neighbors or ih:
            tiles, labels, table = super()._featurize_stack(I, M, slide_mode)
        if self._morph:
            mt, ml, mtab = self._context().morph_tiles_host(I, M, self._morph, self._settings, max_device_bytes=self._device_budget())
            _lib.load().nyxhip_finalize_table(mtab.ctypes.data, mtab.shape[0], mtab.shape[1], mtab.shape[1], C.c_double(self._settings.soft_nan))
            if table is None:
                tiles, labels, table = mt, ml, mtab
            else:
                if not (np.array_equal(mt, tiles) and np.array_equal(ml, labels)):
                    raise RuntimeError("the morphology call and the other calls disagree about the ROIs of the stack")
                table = np.ascontiguousarray(np.hstack([table, mtab]))
        return tiles, labels, table

    def _columns(self):
        requested, ih = self._active()
        names = _lib.column_names(self._mask, self._settings) if self._mask else []
        if self._neighbors:
            names = names + _lib.neighbor_column_names()
        if ih:
            names = names + _lib.ih_column_names()
        if self._morph:
            names = names + _lib.morph_column_names(self._morph)
        angles = [self._settings.glcm_angles[i] for i in range(self._settings.glcm_n_angles)]
        sel = featureset.column_selector(requested, names, angles)
        return [names[i] for i in sel], sel

    def _whole_slide_refusals(self):
        """Whole-slide mode does not serve the morphology codes (the reference builds a four-corner contour there): refused by name,
        before anything touches the device; every other code as in Nyxus."""
        bad = [c for c in self._requested if c in featureset_morph.MORPH_OF]
        if bad:
            raise ValueError(f"feature(s) {bad} are not served in whole-slide mode (single_roi=True, or a directory without label images): "
                             "the morphology classes need label images")
        super()._whole_slide_refusals()
