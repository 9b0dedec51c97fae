"""GPU test of the cloud loader's trip and lane boundaries (roi_features.hip: `issue` / `consume` / `trip_rot`, the rotated trips
of the compact builds, and `trip`, the serial ones of every other build).

A trip is 1024 pixels of the workgroup (four per thread); a ROI's trips are rotated -- the loads of the next trip are issued
while the current one is consumed -- and the first trip is issued in front of the phase-0 clears.  What can go wrong lives at
the boundaries: the last lane of a wave, of a pixel's quarter (256), of a trip (1024), a ROI of whole trips (whose loads behind
the last trip return nothing), one pixel more, one pixel less.  The 2821-px benchmark ROI crosses each of them once.

One batch of ROIs with those pixel counts, three value sets (one per compile-time form of the consume half), the three masks of
the compact builds, on stated extrema (whole-batch launches, the path the benchmark takes) and through the classifier.  Every call
is held to the eight-per-CU carve-out on the library's own launch line (NYXHIP_DEBUG): that is what selects the tier-8 builds, the
ones with the rotated loader (the line names the build, and tests/device_call.py::assert_compact_tier holds it to that); a batch that slid to a generic tier would only test the serial trip."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import device_call as dc
from tests import parity

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 1279, 1280, 2047, 2048, 2049, 2821, 3071, 3072, 3073)
BOX_H = 49                                     # a box of 64 x 49 holds the largest count; the cloud is column-major (x, then y)
SMALL_H = 16                                   # <= 256 px in a box of 16 x 16: size class 0 (roi_small); in columns of 49: class 1
INT_EXACT = ("MIN", "MAX", "RANGE", "MEAN", "INTEGRATED_INTENSITY")


def _roi(n, h, values):
    k = np.arange(n)
    return dict(x=k // h, y=k % h, inten=values[:n].astype(np.uint32))


def _rois(kind):
    """The first n cells of the box in cloud order for every n of COUNTS; the counts up to 256 a second time in columns of 49 (a box
    side above the class-0 bound: the four-wave kernel serves them).  3073 = 62 columns of 49 and 35 cells of the 63rd.
    One ROI departs from that shape: two pixels 33 rows apart in one column -- the smallest count that can have a side above
    the class-0 bound, so that the rotated loader also sees a trip in which three of four waves consume nothing at all."""
    rng = np.random.default_rng({"tiny_nz": 1, "tiny_zero": 2, "wide16": 3}[kind])
    rois = []
    for n in COUNTS:
        for h in ((SMALL_H, BOX_H) if n in (255, 256) else (SMALL_H,) if n < 255 else (BOX_H,)):
            if kind == "wide16":
                v = rng.integers(40000, 44001, n)                  # 16-bit table, vmax >= 2^15: not TINY
            else:
                v = rng.integers(1, 4096, n)                       # no zero, vmax < 2^15: the T, T, T / F, T, T trips
                if kind == "tiny_zero":
                    v[int(rng.integers(0, n))] = 0                 # vmin == 0: the F, F, F trips
            rois.append(_roi(n, h, v))
    far = rng.integers(40000, 44001, 2) if kind == "wide16" else np.array([0 if kind == "tiny_zero" else 7, 4000])
    rois.insert(2, dict(x=np.array([0, 0]), y=np.array([0, 33]), inten=far.astype(np.uint32)))
    return rois


_cache = {}


def _case(kind, mask):
    """Batch, settings and the oracle's table: computed once per (value set, mask), shared, never written to."""
    if kind not in _cache:
        _cache[kind] = (_abi.batch_from_rois(_rois(kind)), _abi.default_settings(8), {})
    b, s, tables = _cache[kind]
    if mask not in tables:
        tables[mask] = po.oracle_featurize(b, mask, s)
        tables[mask].setflags(write=False)
    return b, s, tables[mask]


def _check(G, O, names, b):
    bad = parity.compare_tables(G, O, names, batch=b)
    assert not bad, "\n".join(bad[:20])
    for c in INT_EXACT:                                               # sums of integers: no rounding to allow for
        if c in names:
            j = names.index(c)
            assert np.array_equal(G[:, j], O[:, j]), (c, np.nonzero(G[:, j] != O[:, j])[0][:10])


def test_batch_holds_every_count_and_both_classes():
    b = _abi.batch_from_rois(_rois("tiny_nz"))
    n = np.diff(b.px_offset)
    assert sorted(set(n.tolist())) == list(COUNTS) and b.n_roi == len(COUNTS) + 3
    side = np.maximum(b.bbox_w, b.bbox_h)
    assert side.max() <= 64 and (b.bbox_w * b.bbox_h).max() <= 64 * BOX_H
    assert ((n <= 256) & (side > 32)).sum() == 3 and ((n <= 256) & (side <= 32)).sum() == 4      # class 1 three times, class 0 four times
    assert b.bbox_h[n == 3073][0] == BOX_H and 3073 % BOX_H != 0                                   # a last column that is not full


@pytest.mark.parametrize("mask", [_abi.FAM_INTENSITY | _abi.FAM_GLCM, _abi.FAM_INTENSITY, _abi.FAM_GLCM])
@pytest.mark.parametrize("kind", ["tiny_nz", "tiny_zero", "wide16"])
def test_trip_boundaries_on_stated_extrema(hip_ctx, kind, mask, monkeypatch, capfd):
    b, s, O = _case(kind, mask)
    monkeypatch.setenv("NYXHIP_DEBUG", "1")
    G, rep = dc.device_call(hip_ctx, b, mask, s, stated=True)
    print("largest carve-out", dc.assert_compact_tier(capfd.readouterr().err, mask))
    assert all(r["class"] < 0 for r in rep), rep                      # whole-batch launches, nothing counted
    _check(G, O, _lib.column_names(mask, s), b)


@pytest.mark.parametrize("kind", ["tiny_nz", "tiny_zero", "wide16"])
def test_trip_boundaries_through_the_classifier(hip_ctx, kind, monkeypatch, capfd):
    mask = _abi.FAM_INTENSITY | _abi.FAM_GLCM
    b, s, O = _case(kind, mask)
    monkeypatch.setenv("NYXHIP_DEBUG", "1")
    G, rep = dc.device_call(hip_ctx, b, mask, s, stated=False)
    print("largest carve-out", dc.assert_compact_tier(capfd.readouterr().err, mask))
    assert all(r["class"] >= 0 for r in rep) and sum(r["rois"] for r in rep) == b.n_roi, rep
    _check(G, O, _lib.column_names(mask, s), b)
