"""Cases of the device label scan for volumes (nyxhip_assemble_volumes): small labelled stacks [n, z, y, x] that sit on the seams of the
scan block, share boxes, overflow the label tables and take the several-workgroups cloud form, and the host assembly they are compared
with (nyxus3d.clouds_from_volume + _abi.batch3d_from_rois).  The seam values are read from nyxus_amd/csrc/volscan_plan.h, which
vol_assembly.hip takes its constants from."""
import os
import re
from functools import lru_cache

import numpy as np

from nyxus_amd import _abi
from nyxus_amd.nyxus3d import clouds_from_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_H = os.path.join(ROOT, "nyxus_amd", "csrc", "volscan_plan.h")


@lru_cache(maxsize=None)
def plan_const(name: str) -> int:
    """`constexpr <type> name = <value>;` of volscan_plan.h (decimal, or 1u << k)."""
    with open(PLAN_H) as f:
        m = re.search(r"constexpr \w+ %s = ([^;]+);" % name, f.read())
    v = m.group(1).strip()
    s = re.fullmatch(r"1u << (\d+)", v)
    return 1 << int(s.group(1)) if s else int(v.rstrip("u"))


SCAN_COLS = plan_const("kVsScanCols")
SCAN_ROWS = plan_const("kVsScanRows")
LDS_CAP = plan_const("kVsLdsCap")
CAP_FIRST = plan_const("kVsCapFirst")
CAP_MIN = plan_const("kVsCapMin")
CAP_MAX = plan_const("kVsCapMax")
SLAB_CELLS = plan_const("kVsSlabCells")
TABLE_WORDS = plan_const("kVsTableWords")


def al256(v: int) -> int:
    return (v + 255) & ~255


def first_cap(voxels: int) -> int:
    """The per-volume table a fresh context starts with (vs_cap_first(vs_cap_limit(voxels), 0))."""
    p = 1
    while p < 2 * voxels:
        p <<= 1
    return min(CAP_FIRST, min(max(p, CAP_MIN), CAP_MAX))


def chunk_bytes(shape, inten_dtype, label_dtype) -> int:
    """Budget bytes one staged host volume of `shape` = (z, y, x) takes with its first label table on a fresh context."""
    vox = int(np.prod(shape))
    return al256(vox * np.dtype(inten_dtype).itemsize) + al256(vox * np.dtype(label_dtype).itemsize) + 4 * TABLE_WORDS * first_cap(vox)


def _inten(rng, shape, hi=60000):
    return rng.integers(1, hi, size=shape, dtype=np.uint32)


def _stack(I, L):
    I, L = np.asarray(I), np.asarray(L)
    return (I[None], L[None]) if I.ndim == 3 else (I, L)


def one_voxel():
    return _stack(np.full((1, 1, 1), 5, np.uint32), np.full((1, 1, 1), 7, np.uint32))


def no_label():
    rng = np.random.default_rng(1)
    return _stack(_inten(rng, (3, 4, 5)), np.zeros((3, 4, 5), np.uint32))


def stack_three():
    """Three volumes: the second is empty, label 3 occurs in the first and the third."""
    rng = np.random.default_rng(2)
    I = _inten(rng, (3, 6, 7, 8))
    L = np.zeros((3, 6, 7, 8), np.uint32)
    L[0, 1:4, 2:5, 1:6] = 3
    L[0, 4:6, 0:2, 6:8] = 9
    L[2, 0:2, 0:3, 0:3] = 5
    L[2, 2:6, 3:7, 2:8] = 3
    return I, L


def seam_width(w: int):
    """An ROI that runs from six columns in front of the last column block's seam to the last column, beside a second one."""
    rng = np.random.default_rng(3 + w)
    I = _inten(rng, (2, 3, w))
    L = np.zeros((2, 3, w), np.uint32)
    L[:, 1:3, SCAN_COLS - 6:w] = 21
    L[0, 0, 3:SCAN_COLS - 10] = 22
    return _stack(I, L)


def seam_height(h: int):
    """An ROI over every row of a volume whose height sits at the row count of the scan block."""
    rng = np.random.default_rng(300 + h)
    I = _inten(rng, (2, h, 5))
    L = np.zeros((2, h, 5), np.uint32)
    L[:, :, 1:3] = 31
    L[1, h - 1, 4] = 32
    return _stack(I, L)


def depth_five():
    rng = np.random.default_rng(5)
    I = _inten(rng, (5, 6, 7))
    L = np.zeros((5, 6, 7), np.uint32)
    L[:, 2:4, 3:5] = 41
    L[2, 0, 0] = 42
    return _stack(I, L)


def checkerboard():
    """Two labels interleaved as a 3-D checkerboard in one box: both ROIs have the same box."""
    rng = np.random.default_rng(6)
    I = _inten(rng, (8, 9, 10))
    L = np.zeros((8, 9, 10), np.uint32)
    z, y, x = np.mgrid[0:6, 0:6, 0:6]
    L[1:7, 2:8, 3:9] = np.where((z + y + x) % 2 == 0, 11, 12)
    return _stack(I, L)


def corners():
    """One label in two far corners (its box is the whole volume) around a blob of another."""
    rng = np.random.default_rng(7)
    I = _inten(rng, (9, 10, 11))
    L = np.zeros((9, 10, 11), np.uint32)
    L[0, 0, 0] = 4
    L[8, 9, 10] = 4
    L[3:6, 3:7, 4:8] = 2
    return _stack(I, L)


def shell():
    rng = np.random.default_rng(8)
    I = _inten(rng, (9, 9, 9))
    L = np.zeros((9, 9, 9), np.uint32)
    L[1:8, 1:8, 1:8] = 2
    L[2:7, 2:7, 2:7] = 1
    return _stack(I, L)


def confetti(side: int = 20):
    """Every voxel its own shuffled 32-bit label."""
    rng = np.random.default_rng(9 + side)
    n = side ** 3
    labels = np.unique(rng.integers(1, 2 ** 32, size=2 * n, dtype=np.uint64))[:n].astype(np.uint32)
    assert len(labels) == n
    rng.shuffle(labels)
    return _stack(_inten(rng, (side, side, side)), labels.reshape(side, side, side))


def confetti_blocks(side: int = 12, max_inten: int = 64):
    """2 x 2 x 2 blocks of shuffled 32-bit labels and small intensities: ROIs the level caps of every volume entry admit."""
    rng = np.random.default_rng(90 + side)
    m = side // 2
    labels = np.unique(rng.integers(1, 2 ** 32, size=2 * m ** 3, dtype=np.uint64))[:m ** 3].astype(np.uint32)
    rng.shuffle(labels)
    L = np.repeat(np.repeat(np.repeat(labels.reshape(m, m, m), 2, 0), 2, 1), 2, 2)
    return _stack(rng.integers(1, max_inten, size=L.shape, dtype=np.uint32), L)


def label_values():
    rng = np.random.default_rng(10)
    I = _inten(rng, (4, 5, 12))
    L = np.zeros((4, 5, 12), np.uint32)
    L[:, :, 0:3] = 2 ** 32 - 1
    L[:, :, 4:7] = 1
    L[:, :, 8:11] = 2 ** 31
    L[1, 2, 11] = 2 ** 31 + 1
    return _stack(I, L)


def slab_box():
    """The smallest box of 32 x 32 planes above kVsSlabCells: its cloud takes the several-workgroups form.  Two labels share it, at
    random, so every slab holds hits of both; zero intensities lie under both."""
    rng = np.random.default_rng(11)
    d = SLAB_CELLS // (32 * 32) + 1
    shape = (d + 2, 33, 34)
    I = _inten(rng, shape)
    I[rng.random(shape) < 0.2] = 0
    L = np.zeros(shape, np.uint32)
    L[1:d + 1, 0:32, 1:33] = rng.choice(np.array([0, 77, 78], np.uint32), size=(d, 32, 32), p=[0.3, 0.4, 0.3])
    L[1, 0, 1] = 77                                        # the box of 77 is the full window
    L[d, 31, 32] = 77
    return _stack(I, L)


def zero_intensity():
    rng = np.random.default_rng(12)
    I = _inten(rng, (4, 5, 6))
    L = np.zeros((4, 5, 6), np.uint32)
    L[1:3, 1:4, 1:5] = 6
    I[1:3, 1:4, 1:3] = 0
    L[3, 4, 5] = 8
    I[3, 4, 5] = 0                                         # an ROI whose only voxel has intensity 0
    return _stack(I, L)


def small_types(inten_dtype, label_dtype):
    """One small two-volume stack in a given pair of element types (values within 8 bits)."""
    rng = np.random.default_rng(13)
    I = rng.integers(0, 256, size=(2, 5, 6, 7), dtype=np.uint32)
    L = np.zeros((2, 5, 6, 7), np.uint32)
    L[0, 1:4, 1:5, 2:6] = 200
    L[0, 0, 0, 0:3] = 255
    L[1, 2:5, 0:3, 0:4] = 17
    L[1, 4, 5, 6] = 200
    return I.astype(inten_dtype), L.astype(label_dtype)


DTYPES = (np.uint8, np.uint16, np.uint32)

CASES = {
    "one_voxel": one_voxel,
    "no_label": no_label,
    "stack_three": stack_three,
    "seam_w255": lambda: seam_width(SCAN_COLS - 1),
    "seam_w256": lambda: seam_width(SCAN_COLS),
    "seam_w257": lambda: seam_width(SCAN_COLS + 1),
    "seam_h_minus": lambda: seam_height(SCAN_ROWS - 1),
    "seam_h_exact": lambda: seam_height(SCAN_ROWS),
    "seam_h_plus": lambda: seam_height(SCAN_ROWS + 1),
    "depth_five": depth_five,
    "checkerboard": checkerboard,
    "corners": corners,
    "shell": shell,
    "confetti": confetti,
    "label_values": label_values,
    "slab_box": slab_box,
    "zero_intensity": zero_intensity,
}
# the cases that go through the five volume entries: seams, checkerboard, confetti at a size and intensities the level caps admit
ENTRY_CASES = {
    "seam_w257": lambda: _small_inten(seam_width(SCAN_COLS + 1)),
    "checkerboard": lambda: _small_inten(checkerboard()),
    "confetti_blocks": confetti_blocks,
}


def _small_inten(case):
    I, L = case
    return (I % 63 + 1).astype(np.uint32), L


def host_assembly(I: np.ndarray, L: np.ndarray):
    """The host assembly of a stack: (HostBatch3D, volume index of every row), rows in (volume, ascending label) order."""
    rois, vol_of = [], []
    for v in range(I.shape[0]):
        cl = clouds_from_volume(I[v], L[v])
        rois += cl
        vol_of += [v] * len(cl)
    return _abi.batch3d_from_rois(rois), np.asarray(vol_of, np.uint32)
