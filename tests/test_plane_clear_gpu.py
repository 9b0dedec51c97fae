"""GPU test of the phase-0 clear of the 8-bit co-occurrence plane (roi_features.hip: 16-byte stores over area + 64 bytes, rounded up).

The plane of a workgroup lies where the plane of the workgroup before it lay, and nothing but phase 0 zeroes it: a cell of the box
that the ROI does not own, the 64 zero bytes behind the last row, are whatever the last tenant left unless the clear reaches them --
and a clear that runs past the plane's region would wipe the scratch behind it.  So a call of 61 x 61 squares with every cell
non-zero first fills the planes of every workgroup slot of the device; then ONE batch, several hundred ROIs long, of such squares,
boxes with holes whose areas are 0, 1, 5 and 15 modulo 16 (and 3, 4 and 9), and squares again.  The GLCM columns of the boxes
would show a cell left dirty.  Masks 3 and 2 run the clear; mask 1 has no plane and is the control."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import device_call as dc
from tests import parity

pytestmark = pytest.mark.gpu

# (w, h, pixels): areas 320 = 0, 289 = 1, 437 = 5, 399 = 15 (mod 16); 340 = 4 with 300 px, 323 = 3, 441 = 9.  More than 256 px each:
# the four-wave builds, not the wave-per-ROI kernel of the smallest size class
BOXES = [(16, 20, 290), (17, 17, 262), (19, 23, 395), (19, 21, 360), (17, 20, 300), (17, 19, 291), (21, 21, 400)]
REPS = 30
VMAX = 1024                                    # a 1024-entry counting table: the 3721-px square keeps the eight-per-CU carve-out
SLOTS = 256 * 8 + 256                          # more workgroups than the device holds at once


def _square(rng):
    k = np.arange(61 * 61)
    return dict(x=k // 61, y=k % 61, inten=rng.integers(1, VMAX, 61 * 61).astype(np.uint32))


def _box(w, h, n, rng):
    """n cells of a w x h box in cloud order (x outer); the four corners stay, so the box is the bounding box."""
    cells = np.arange(w * h)
    corners = np.array([0, h - 1, (w - 1) * h, w * h - 1])
    rest = np.setdiff1d(cells, corners)
    k = np.sort(np.concatenate([corners, rng.choice(rest, n - 4, replace=False)]))
    return dict(x=k // h, y=k % h, inten=rng.integers(1, VMAX, n).astype(np.uint32))


def _rois():
    rng = np.random.default_rng(33)
    rois = []
    for _ in range(REPS):
        rois.append(_square(rng))
        rois += [_box(w, h, n, rng) for w, h, n in BOXES]
        rois.append(_square(rng))
    return rois


_cache = {}


def _case(mask):
    if "b" not in _cache:
        _cache["b"] = _abi.batch_from_rois(_rois())
        sq = _square(np.random.default_rng(34))
        _cache["dirty"] = _abi.batch_from_rois([sq] * SLOTS)
    b, s = _cache["b"], _abi.default_settings(8)
    if mask not in _cache:
        _cache[mask] = po.oracle_featurize(b, mask, s)
        _cache[mask].setflags(write=False)
    return b, _cache["dirty"], s, _cache[mask]


def test_batch_shape():
    b = _abi.batch_from_rois(_rois())
    assert b.n_roi == REPS * (len(BOXES) + 2) >= 200
    area = (b.bbox_w * b.bbox_h)[1:1 + len(BOXES)]
    assert [int(a) % 16 for a in area] == [0, 1, 5, 15, 4, 3, 9]
    n = np.diff(b.px_offset)
    assert n.min() > 256 and n[0] == 3721 == b.bbox_w[0] * b.bbox_h[0] and (n[1:1 + len(BOXES)] < area).all()
    assert b.inten.min() >= 1                                          # every cell of a square gets a non-zero level


@pytest.mark.parametrize("mask", [_abi.FAM_INTENSITY | _abi.FAM_GLCM, _abi.FAM_GLCM, _abi.FAM_INTENSITY])
def test_planes_are_clean_behind_full_squares(hip_ctx, mask, monkeypatch, capfd):
    b, dirty, s, O = _case(mask)
    dc.device_call(hip_ctx, dirty, _abi.FAM_INTENSITY | _abi.FAM_GLCM, s)        # every slot's plane: 3721 non-zero cells
    monkeypatch.setenv("NYXHIP_DEBUG", "1")
    capfd.readouterr()
    G, rep = dc.device_call(hip_ctx, b, mask, s, prime=False)
    print("largest carve-out", dc.assert_compact_tier(capfd.readouterr().err, mask))
    assert all(r["class"] < 0 for r in rep), rep                      # whole-batch launches: the workgroups run in batch order
    bad = parity.compare_tables(G, O, _lib.column_names(mask, s), batch=b)
    assert not bad, "\n".join(bad[:20])
