"""Helpers of the GPU tests that drive the device entry the way the benchmark does: a batch in device memory, its extrema stated
(whole-batch launches, nothing counted) or withheld (the classifier derives the classes), the output table in a torch buffer."""
import re

import numpy as np

from nyxus_amd import _abi

OCC8_LDS = 20480                               # bytes of LDS a workgroup may carve out with eight per CU (plan_features_launch)
_LAUNCH = re.compile(r"features launch: g16 (\d+) dense8 (\d+) cnt16 (\d+) ng_cap \d+ app \d+ total (\d+) mask (\d+)")
_BUILD = re.compile(r"features launch: .* build (small|tier (\d+) fam (\d+) win (\d+) c16 (\d+) split (\d+) d8 (\d+) nw (\d+) defer (\d+))$", re.M)
BUILD_KEYS = ("tier", "fam", "win", "c16", "split", "d8", "nw", "defer")
COMPACT_FAM = {_abi.FAM_INTENSITY | _abi.FAM_GLCM: 1, _abi.FAM_INTENSITY: 2, _abi.FAM_GLCM: 3}      # the compile-time family sets
_PRIME = []


def to_device(b):
    """The arrays of a HostBatch as torch tensors on cuda:0 and the C struct that points at them (keep both alive)."""
    import torch
    dev = torch.device("cuda", 0)
    keep = {k: torch.from_numpy(getattr(b, k).view({2: np.int16, 4: np.int32, 8: np.int64}[getattr(b, k).dtype.itemsize])).to(dev)
            for k in ("px_offset", "x", "y", "inten", "bbox_w", "bbox_h", "min_inten", "max_inten")}
    cb = b.c_struct()
    for k, t in keep.items():
        setattr(cb, k, t.data_ptr())
    cb.slide_min = None; cb.slide_max = None; cb.memory = _abi.MEM_DEVICE
    return cb, keep


def enqueue(ctx, b, mask, s, stated=True):
    """featurize_device_async over the batch -> (output tensor, what keeps the inputs alive).  Nothing is synchronised."""
    import torch
    cb, keep = to_device(b)
    if not stated:
        cb.max_px = cb.max_bbox_area = cb.max_bbox_side = 0           # no statement: the classifier derives the classes
    ncol = ctx.n_columns(mask, s)
    out = torch.full((b.n_roi, ncol), -1.0, dtype=torch.float64, device=torch.device("cuda", 0))
    ctx.featurize_device_async(cb, mask, s, out.data_ptr(), ncol)
    return out, (cb, keep)


def prime_census(ctx, mask, s):
    """A call of one class-1 ROI on stated extrema: resets the context's census of the smallest size class."""
    if not _PRIME:
        k = np.arange(300)
        _PRIME.append(_abi.batch_from_rois([dict(x=k // 49, y=k % 49, inten=(k + 1).astype(np.uint32))]))
    device_call(ctx, _PRIME[0], mask, s, True, prime=False)


def device_call(ctx, b, mask, s, stated=True, prime=True):
    """One call -> (table, launch report).  On stated extrema a call of one class-1 ROI goes first: it resets the context's census of
    the smallest size class, which the calls before left in whatever state and which decides between whole-batch launches and lists."""
    if stated and prime:
        prime_census(ctx, mask, s)
    out, keep = enqueue(ctx, b, mask, s, stated)
    rep = ctx.launch_report()
    ctx.sync()
    del keep
    return out.cpu().numpy(), rep


def launch_lines(err):
    """(g16, dense8, cnt16, total, mask) of every feature launch the library reported on stderr under NYXHIP_DEBUG=1."""
    return [tuple(int(g) for g in m.groups()) for m in _LAUNCH.finditer(err)]


def launch_builds(err):
    """What every feature launch reported as its engine: "small" (the wave-per-ROI kernel), or the template arguments of the build of
    roi_features_kernel as a dict over BUILD_KEYS.  One entry per launch line, in the order of launch_lines."""
    return ["small" if m.group(1) == "small" else dict(zip(BUILD_KEYS, (int(g) for g in m.groups()[1:]))) for m in _BUILD.finditer(err)]


def assert_compact_tier(err, mask):
    """Every feature launch of the call had the 16-bit tables and the 8-bit plane where it has any, and a carve-out that fits eight
    times per CU: the conditions under which plan_features_launch picks the tier-8 build of the mask's family set for a cloud launch
    -- and that build (or the wave-per-ROI kernel) is what the line names."""
    lines = launch_lines(err)
    assert lines, err[-2000:]
    builds = launch_builds(err)
    assert len(builds) == len(lines), err[-2000:]
    for b in builds:
        assert b == "small" or (b["tier"], b["fam"], b["win"], b["nw"], b["defer"]) == (8, COMPACT_FAM[mask], 0, 4, int(bool(mask & _abi.FAM_INTENSITY))), (builds, err[-2000:])
    for g16, dense8, cnt16, total, lmask in lines:
        assert lmask == mask and g16 == 0 and total <= OCC8_LDS, (lines, err[-2000:])
        assert cnt16 == 1 or not (mask & _abi.FAM_INTENSITY), lines
        assert dense8 == 1 or not (mask & _abi.FAM_GLCM), lines
    return max(l[3] for l in lines)
