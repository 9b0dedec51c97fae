"""The column catalogue over the whole 26-bit mask space (bits 0 .. 25 without the unassigned 12 and 14), the parts that need no GPU:
every family owns one set of names, a mask's columns are the full list filtered to its families in that order, and a bit that is not
a family adds no column.  Also the self-checks of the batch tests/test_mask_lattice_gpu.py runs."""
import ctypes as C

import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from tests import mask_lattice_cases as mc

CONFIGS = [pytest.param(mc.settings_a, id="a"), pytest.param(mc.settings_b, id="b")]
CONFIGS += [pytest.param(lambda na=na, nf=nf: mc.settings_b(na, nf), id=f"na{na}-nf{nf}") for na in (1, 2, 3, 4) for nf in (0, 4, 16)]


def test_the_family_bits():
    assert len(mc.BITS) == 24 and len(set(mc.BITS)) == 24 and all(b & (b - 1) == 0 for b in mc.BITS)
    assert sorted(mc.BITS + [1 << k for k in mc.UNASSIGNED]) == [1 << k for k in range(32)]
    assert mc.FULL & _abi.FAM_ALL == _abi.FAM_ALL and bin(_abi.FAM_ALL).count("1") == 12
    g = mc.masks()
    assert g == mc.masks()                                                       # deterministic
    assert len(g["singles"]) == 24 and len(g["leave_one_out"]) == 24 and g["full"] == [mc.FULL]
    assert len(g["glcm_span"]) == 3 * len(mc.BEHIND_INTENSITY) and len(g["random"]) == 48
    assert len(g["interleave"]) == len(set(g["interleave"])) == 16 + 3 * 128
    assert all(0 < m <= mc.FULL and not (m & ~mc.FULL) for ms in g.values() for m in ms)
    assert mc.MASK_DEPENDENT == {}


@pytest.mark.parametrize("make", CONFIGS)
def test_every_mask_is_the_full_list_filtered(make):
    s = make()
    lib = _lib.load()
    full = _lib.column_names(mc.FULL, s)
    assert len(full) == len(set(full)) == lib.nyxhip_n_columns(mc.FULL, C.byref(s))
    single = {b: _lib.column_names(b, s) for b in mc.BITS}
    owner = {}
    for b, names in single.items():
        assert len(names) == lib.nyxhip_n_columns(b, C.byref(s))
        for n in names:
            assert n not in owner, (n, hex(b), hex(owner[n]))
            owner[n] = b
    assert sorted(owner) == sorted(full)                                         # the 24 single-bit lists partition the full list
    assert all(len(v) > 0 for b, v in single.items() if not (b == _abi.FAM_GABOR and s.gabor_n_filters == 0))
    # the families between the intensity block and GLCM (kBehindIntensity), from the column order
    first = {b: full.index(single[b][0]) for b in mc.BITS if single[b]}
    behind = [b for b in first if first[_abi.FAM_INTENSITY] < first[b] < first[_abi.FAM_GLCM]]
    assert sorted(behind) == sorted(mc.BEHIND_INTENSITY)
    rng = np.random.default_rng(2000)
    more = [int(sum(b for b in mc.BITS if rng.random() < p)) for p in rng.choice([0.2, 0.5, 0.8], 2000)]
    todo = [m for ms in mc.masks().values() for m in ms] + [m for m in more if m]
    assert len(todo) > 2500
    for mask in todo:
        want = [n for n in full if owner[n] & mask]
        assert lib.nyxhip_n_columns(mask, C.byref(s)) == sum(len(single[b]) for b in mc.bits_of(mask)) == len(want), hex(mask)
        assert _lib.column_names(mask, s) == want, hex(mask)


@pytest.mark.parametrize("make", CONFIGS[:2])
def test_a_bit_that_is_no_family_adds_no_column(make):
    """Bits 12, 14 and 26 .. 31: nyxhip_n_columns counts nothing for them and nyxhip_column_name has no column behind the last one of
    the valid part.  (That a featurize call REFUSES such a mask needs a context: tests/test_mask_lattice_gpu.py.)"""
    s = make()
    lib = _lib.load()
    buf = C.create_string_buffer(128)
    for k in mc.UNASSIGNED:
        bad = 1 << k
        assert lib.nyxhip_n_columns(bad, C.byref(s)) == 0
        assert lib.nyxhip_column_name(bad, C.byref(s), 0, buf, 128) == 1        # NYXHIP_ERR_INVALID_ARG
        for good in (_abi.FAM_EULER, mc.FULL, _abi.FAM_GLCM | _abi.FAM_CHORDS):
            n = lib.nyxhip_n_columns(good, C.byref(s))
            assert lib.nyxhip_n_columns(good | bad, C.byref(s)) == n
            assert lib.nyxhip_column_name(good | bad, C.byref(s), n - 1, buf, 128) == 0 and buf.value.decode() == _lib.column_names(good, s)[-1]
            assert lib.nyxhip_column_name(good | bad, C.byref(s), n, buf, 128) == 1


def test_the_batch_reaches_every_path():
    b, keys = mc.lattice_batch()
    assert 15 <= b.n_roi <= 24 and len(keys) == b.n_roi
    cl = mc.classes(b)
    L = mc.listed(b)
    print("classes:", dict(zip(keys, cl)))
    print("listed:", {k: [keys[r] for r in v] for k, v in L.items()})
    assert sorted(set(cl)) == [0, 2, 3, 4, 6, 7, 8]
    # the restated class rule at its bounds (roi_kernel.h: kClassPx, kClassSide)
    assert [mc.roi_class(*a) for a in ((256, 32, 32, 0), (257, 32, 8, 0), (256, 33, 1, 0), (4096, 64, 64, 16383), (4096, 64, 64, 16384),
                                       (4097, 64, 65, 0), (16384, 128, 128, 65535), (16384, 128, 128, 65536), (32768, 256, 128, 0),
                                       (32769, 256, 256, 0), (100, 257, 1, 0), (65536, 256, 256, 0))] == [0, 2, 2, 2, 3, 4, 5, 7, 6, 8, 8, 9]
    it, lab, rows = mc.tile_subset(b, keys)
    assert lab.max() == max(rows) + 1 and len(np.unique(lab)) == len(rows) + 1
