"""GPU test of the ONE per-call clear of the matrix orders and the pending closing flags (nyxhip_dispatch.hip: d_roi_words) and of what a
call leaves to stream order around the closing launch of the deferred intensity columns (intensity_close_kernel).  (Named for the
closing lane that would have run that launch beside glcm_features_kernel8: measured and not kept, profiles/r33_per_roi_once.txt;
the cases are the ones a second stream would have had to survive, and they hold for one stream as well.)

What a missing wait, or a clear that misses the second table or reaches into the wrong one, would show: deferred intensity columns
of a row that are still the zeroes of phase 0 when somebody reads the table -- the next call on the context, the next launch group
of the call, a family whose columns lie behind the intensity block, the caller's own kernel on the stream -- a closing launch that
consumed the records of the wrong call, GLCM columns derived from a stale matrix order, or a flag still pending when the call is
through.  Every case holds all columns to the oracle and reads the flags back (Context.roi_words): none may be left set."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import device_call as dc
from tests import parity

pytestmark = pytest.mark.gpu

INT_GLCM = _abi.FAM_INTENSITY | _abi.FAM_GLCM


def _box(w, h, rng, hi=4096):
    k = np.arange(w * h)
    return dict(x=k // h, y=k % h, inten=rng.integers(1, hi, w * h).astype(np.uint32))


_cache = {}


def _batch(name):
    """600 ROIs each.  a, b: boxes of 17 x 20 (size class 1: the four-wave builds, deferred closing) with different pixels;
    mixed: 300 boxes of 10 x 10 (size class 0, the wave-per-ROI kernel) and 300 of 17 x 20, interleaved."""
    if name not in _cache:
        rng = np.random.default_rng({"a": 41, "b": 42, "mixed": 43}[name])
        if name == "mixed":
            rois = [_box(10, 10, rng) if i % 2 == 0 else _box(17, 20, rng) for i in range(600)]
        else:
            rois = [_box(17, 20, rng, hi=4096 if name == "a" else 300) for _ in range(600)]
        _cache[name] = _abi.batch_from_rois(rois)
    return _cache[name]


def _oracle(name, mask, s):
    key = (name, mask)
    if key not in _cache:
        _cache[key] = po.oracle_featurize(_batch(name), mask, s)
        _cache[key].setflags(write=False)
    return _cache[key]


def _hold(G, name, mask, s):
    names = _lib.column_names(mask, s)
    assert mask != INT_GLCM or len(names) == 185
    bad = parity.compare_tables(G, _oracle(name, mask, s), names, batch=_batch(name))
    assert not bad, "\n".join(bad[:20])


def _no_flag_pending(ctx, n_roi, live_orders=None):
    """The tables of the last call on the context, read back behind a sync: no closing flag is left set; the matrix orders are those
    of this call (every ROI of these batches is live: one order per ROI that went through the split GLCM launch)."""
    orders, flags = ctx.roi_words(n_roi)
    assert flags == 0, (orders, flags)
    if live_orders is not None:
        assert orders == live_orders, (orders, live_orders)


def test_two_calls_back_to_back(hip_ctx):
    s = _abi.default_settings(8)
    dc.device_call(hip_ctx, _batch("a"), INT_GLCM, s)                  # (the census of the smallest class: whole-batch launches below)
    out_a, keep_a = dc.enqueue(hip_ctx, _batch("a"), INT_GLCM, s)
    out_b, keep_b = dc.enqueue(hip_ctx, _batch("b"), INT_GLCM, s)      # straight behind: its flag clear and its records meet call a's closing
    hip_ctx.sync()
    _no_flag_pending(hip_ctx, 600, live_orders=600)
    _hold(out_a.cpu().numpy(), "a", INT_GLCM, s)
    _hold(out_b.cpu().numpy(), "b", INT_GLCM, s)


@pytest.mark.parametrize("stated", [True, False])
def test_two_classes_in_one_call(hip_ctx, stated):
    """Stated extrema: the filtered pair of launches (class 0, then the rest with the one GLCM feature launch of the call behind it);
    withheld: exact lists, one launch group per class."""
    s = _abi.default_settings(8)
    G, rep = dc.device_call(hip_ctx, _batch("mixed"), INT_GLCM, s, stated=stated)
    assert len(rep) >= 2 and all((r["class"] < 0) == stated for r in rep), rep
    _no_flag_pending(hip_ctx, 600)
    _hold(G, "mixed", INT_GLCM, s)


def test_an_outline_family_behind_the_intensity_block(hip_ctx):
    """EULER_NUMBER lies between the intensity block and GLCM; its kernels are enqueued behind the feature launches.  The 185 other
    columns are held to the oracle (which does not serve the family), the family's own to a call that asks for it alone."""
    s = _abi.default_settings(8)
    mask = INT_GLCM | _abi.FAM_EULER
    G, rep = dc.device_call(hip_ctx, _batch("a"), mask, s)
    _no_flag_pending(hip_ctx, 600, live_orders=600)
    names = _lib.column_names(mask, s)
    j = names.index("EULER_NUMBER")
    assert names[:j] + names[j + 1:] == _lib.column_names(INT_GLCM, s)
    _hold(np.delete(G, j, axis=1), "a", INT_GLCM, s)
    alone, _ = dc.device_call(hip_ctx, _batch("a"), _abi.FAM_EULER, s)
    assert np.array_equal(G[:, j], alone[:, 0])


def test_the_callers_kernel_right_behind_the_call():
    """The table is read by a torch kernel enqueued on the call's stream with nothing between: stream order is all the caller has."""
    import torch
    s = _abi.default_settings(8)
    ctx = _lib.Context(0)
    try:
        ts = torch.cuda.Stream()
        ctx.set_stream(ts.cuda_stream)
        with torch.cuda.stream(ts):
            first = dc.enqueue(ctx, _batch("b"), INT_GLCM, s)          # (census; and something in flight in front of the call under test)
            out, keep = dc.enqueue(ctx, _batch("a"), INT_GLCM, s)
            copy = out * 1.0                                           # the caller's kernel: no sync, no event in between
        ts.synchronize()
        _no_flag_pending(ctx, 600, live_orders=600)
        del first, keep
        _hold(copy.cpu().numpy(), "a", INT_GLCM, s)
    finally:
        ctx.close()
