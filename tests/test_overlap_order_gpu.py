"""GPU tests of the overlapped order of roi_features_body (nyxus_amd/csrc/roi_features.hip): in INTENSITY | GLCM launches
at up to 16 levels the central-sum sweep runs in front of the counting engine, and the order-statistics chain (wave 0), the n-bin bounds
with the entropy (wave 1) and the co-occurrence sweep share one barrier interval, the rows divided by glcm_row_bounds (1 : 3 : 8 : 8 of
twenty: in a box of 5 .. 24 rows waves 0 and 1 get none or one).  Whole rows go against the CPU oracle through tests/parity.py.

Every cloud but the wide-range one runs in the four-wave kernel from LDS (read off the launch report: size classes 1 and 2; the
wide-range ROI only makes the call take exact class lists).  The carve-out's statement about the order (LdsLayout::overlap) is read off
the launch line of NYXHIP_DEBUG=1: the big batch gets the overlap, the batch of 16 levels beside clouds of about 300 px -- four matrices
of 17 x 17 words would run on into the counting table -- keeps the serial order."""
import re

import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from oracle import pyoracle as po
from tests import parity

INT_GLCM = _abi.FAM_INTENSITY | _abi.FAM_GLCM


def box(w, h, rng, zeros=False, lo=1, hi=4096):
    """A full w x h box of random 12-bit intensities; zeros: a third of the pixels at intensity 0."""
    v = rng.integers(lo, hi, w * h).astype(np.uint32)
    if zeros:
        v[rng.permutation(w * h)[:(w * h) // 3]] = 0
    k = np.arange(w * h)
    return dict(x=k % w, y=k // w, inten=v)


def disk(r, rng):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    m = xx * xx + yy * yy <= r * r
    return dict(x=xx[m] + r, y=yy[m] + r, inten=rng.integers(1, 4096, int(m.sum())).astype(np.uint32))


def wide_roi(rng):
    """A range beyond the 16-bit tables in a box 40 px wide: with it in the batch the call takes exact class lists."""
    v = rng.integers(1, 70000, 400).astype(np.uint32)
    v[0], v[1] = 1, 69999
    k = np.arange(400)
    return dict(x=k % 40, y=k // 40, inten=v)


def build_big():
    rng = np.random.default_rng(2026)
    rois = [box(64, h, rng) for h in range(5, 25)]                              # waves 0 and 1: no row or one row
    rois += [box(64, h, rng) for h in (39, 40, 41, 61, 64)]
    rois += [box(w, h, rng) for w in (65, 100, 128) for h in (3, 4, 5, 6, 7, 8, 61)]   # two columns per lane
    rois += [disk(30, rng)]
    rois += [box(64, h, rng, zeros=True) for h in (5, 13, 24, 40)] + [box(100, 7, rng, zeros=True)]
    const = box(64, 8, rng); const["inten"][:] = 7                             # degenerate: the waves skip their rows inside the interval
    blank = box(64, 8, rng); blank["inten"][:] = 0                             # blank: no sweep, no chain, the same barriers
    rois += [const, box(64, 8, rng), blank, box(64, 9, rng)]
    return rois + [wide_roi(rng)]


def build_serial():
    """About 300 px a cloud: at 16 levels the matrices (4 x 17 x 17 words from the value buffer on) reach into the counting table."""
    rng = np.random.default_rng(77)
    rois = [box(64, 5, rng), box(60, 5, rng), box(40, 8, rng), box(64, 5, rng, zeros=True), box(33, 9, rng), box(65, 4, rng)]
    const = box(64, 5, rng); const["inten"][:] = 300
    blank = box(64, 5, rng); blank["inten"][:] = 0
    return rois + [const, blank, box(50, 6, rng), wide_roi(rng)]


BIG, SERIAL = build_big(), build_serial()
_ORACLE = {}


def settings(gd, angles=(0, 45, 90, 135), symmetric=False, offset=1):
    s = _abi.default_settings(gd)
    s.glcm_n_angles = len(angles)
    for i, a in enumerate(angles):
        s.glcm_angles[i] = a
    s.glcm_symmetric = 1 if symmetric else 0
    s.glcm_offset = offset
    return s


def run(ctx, rois, s, capfd, monkeypatch, key):
    """The batch on the GPU against the oracle; returns the overlap words of the feature launches' debug lines."""
    b = _abi.batch_from_rois(rois)
    monkeypatch.setenv("NYXHIP_DEBUG", "1")
    capfd.readouterr()
    G = ctx.featurize_host(b, INT_GLCM, s)
    err = capfd.readouterr().err
    monkeypatch.delenv("NYXHIP_DEBUG")
    if key not in _ORACLE:
        _ORACLE[key] = po.oracle_featurize(b, INT_GLCM, s)
    bad = parity.compare_tables(G, _ORACLE[key], _lib.column_names(INT_GLCM, s), batch=b)
    assert not bad, "\n".join(bad[:20])
    rep = ctx.launch_report()
    print(rep)
    assert all(r["class"] >= 0 and r["workspace"] == 0 for r in rep), rep                   # exact classes, from LDS
    assert sum(r["rois"] for r in rep) == len(rois), rep
    assert all(r["size_class"] in (1, 2) for r in rep), rep                                 # the four-wave kernel, nobody else
    return [int(m) for m in re.findall(r"features launch:.* overlap (\d)", err)]


VARIANTS = {"usual": dict(), "symmetric": dict(symmetric=True), "angle_0": dict(angles=(0,)), "angles_45_135": dict(angles=(45, 135))}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_overlapped_launches_match_the_oracle(hip_ctx, capfd, monkeypatch, variant):
    flags = run(hip_ctx, BIG, settings(8, **VARIANTS[variant]), capfd, monkeypatch, ("big", variant))
    assert flags.count(1) >= 2, flags                  # size classes 1 and 2 of the 16-bit tables: both carve-outs allow the overlap


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["usual", "symmetric"])
def test_serial_launches_match_the_oracle(hip_ctx, capfd, monkeypatch, variant):
    flags = run(hip_ctx, SERIAL, settings(16, **VARIANTS[variant]), capfd, monkeypatch, ("serial", variant))
    assert flags and 1 not in flags, flags             # the matrices would reach the counting table: the serial order


@pytest.mark.gpu
def test_generic_loop_inside_the_shared_interval(hip_ctx, capfd, monkeypatch):
    """Offset 2: rows dealt to the waves round-robin, plain matrices -- in the same interval as the chain."""
    rng = np.random.default_rng(5)
    rois = [box(64, h, rng) for h in (11, 12, 40)] + [box(100, 9, rng), box(64, 20, rng, zeros=True), wide_roi(rng)]
    flags = run(hip_ctx, rois, settings(8, offset=2), capfd, monkeypatch, ("offset2",))
    assert 1 in flags, flags


@pytest.mark.gpu
def test_a_box_129_wide(hip_ctx):
    """129 x 3: beyond the two-columns-per-lane form.  Its size class (sides up to 256) belongs to the large-ROI path, so the row is
    held to the oracle whatever kernel serves it."""
    rng = np.random.default_rng(6)
    rois = [box(129, 3, rng), box(64, 12, rng)]
    b = _abi.batch_from_rois(rois)
    s = settings(8)
    G = hip_ctx.featurize_host(b, INT_GLCM, s)
    bad = parity.compare_tables(G, po.oracle_featurize(b, INT_GLCM, s), _lib.column_names(INT_GLCM, s), batch=b)
    assert not bad, "\n".join(bad[:20])
    print(hip_ctx.launch_report())
