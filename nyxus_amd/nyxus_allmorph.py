"""nyxus_amd.NyxusAllMorphology -- class `NyxusMorphology` plus POLYGONALITY_AVE, HEXAGONALITY_AVE, HEXAGONALITY_STDDEV and with them the
group *ALL_MORPHOLOGY* (featureset_allmorph).  `Nyxus` and `NyxusMorphology` keep refusing the three codes and the group; this class
serves them through nyxhip_hexpoly_tiles with `neighbor_distance` and puts their table to the right of the others.  Columns are
selected by name, in enum order.  Every entry a request touches runs the contour chain of its own: there is no fused call."""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np

from . import _lib, featureset, featureset_allmorph
from .nyxus_morph import NyxusMorphology


class NyxusAllMorphology(NyxusMorphology):
    def _set_features(self, features: List[str]):
        """self._hexpoly: a hexagonality / polygonality code is requested; everything else as in NyxusMorphology._set_features."""
        self._features = list(features)
        full, self._morph, self._hexpoly, self._requested = featureset_allmorph.expand_all_morph(self._features)
        self._mask, self._neighbors = featureset.split_neighbors(full)
        self._ih = featureset.split_ih(full)

    def _featurize_stack(self, I: np.ndarray, M: np.ndarray, slide_mode: int):
        """The tables of NyxusMorphology._featurize_stack and, to their right, the three columns of nyxhip_hexpoly_tiles (one image per
        tile, neighbors counted at `neighbor_distance`).  The call runs on the first context only."""
        _, ih = self._active()
        tiles = labels = table = None
        if self._mask or self._neighbors or ih or self._morph:
            tiles, labels, table = super()._featurize_stack(I, M, slide_mode)
        if self._hexpoly:
            ht, hl, htab = self._context().hexpoly_tiles_host(I, M, int(self._env["neighbor_distance"]), self._settings,
                                                              max_device_bytes=self._device_budget())
            _lib.load().nyxhip_finalize_table(htab.ctypes.data, htab.shape[0], htab.shape[1], htab.shape[1], C.c_double(self._settings.soft_nan))
            if table is None:
                tiles, labels, table = ht, hl, htab
            else:
                if not (np.array_equal(ht, tiles) and np.array_equal(hl, labels)):
                    raise RuntimeError("the hexagonality / polygonality call and the other calls disagree about the ROIs of the stack")
                table = np.ascontiguousarray(np.hstack([table, htab]))
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
        if self._hexpoly:
            names = names + _lib.hexpoly_column_names()
        angles = [self._settings.glcm_angles[i] for i in range(self._settings.glcm_n_angles)]
        sel = featureset.column_selector(requested, names, angles)
        return [names[i] for i in sel], sel

    def _whole_slide_refusals(self):
        """Whole-slide mode does not serve the three codes (a slide is one ROI: it has no neighbor): refused by name, before anything
        touches the device; every other code as in NyxusMorphology."""
        bad = [c for c in self._requested if c in featureset_allmorph.HEXPOLY]
        if bad:
            raise ValueError(f"feature(s) {bad} are not served in whole-slide mode (single_roi=True, or a directory without label images): "
                             "the hexagonality / polygonality class needs label images")
        super()._whole_slide_refusals()
