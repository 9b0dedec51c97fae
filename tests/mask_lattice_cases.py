"""Inputs of tests/test_mask_lattice_cpu.py and tests/test_mask_lattice_gpu.py: the 26 family bits, two settings at a soft_nan that is
not 0.0, one batch of ROIs that reaches every launch path (every size class of roi_kernel.h: roi_class, both table widths of the odd
classes, each of the five deferred lists of nyxhip_contour.hip) and deterministic lists of family masks.  The tests hold every family
block of every mask against the block of that family's call alone (a row never depends on companions)."""
import itertools

import numpy as np

from nyxus_amd import _abi
from tests import caliper_cases, chords_cases, erosion_cases, outline_cases, outline_ref, soft_nan_cases as sc, synth
from tests.radial_cases import _mask_roi, disc

SOFT_NAN = sc.SOFT_NAN
POISON = -12345.0

# ---- the 26 family bits ---------------------------------------------------------------------------------------------------------------
BIT_NAMES = ["INTENSITY", "GLCM", "GLRLM", "GLSZM", "NGTDM", "GABOR", "ZERNIKE", "GLDZM", "GLDM", "NGLDM", "SMOMS", "IMOMS", "RADIAL", "FRACTAL",
             "EULER", "ROI_RADIUS", "FERET", "MARTIN", "NASSENSTEIN", "CHORDS", "ELLIPSE", "EROSION", "CIRCLES", "GEODETIC"]
BITS = [getattr(_abi, "FAM_" + n) for n in BIT_NAMES]
NAME_OF = dict(zip(BITS, BIT_NAMES))
FULL = 0
for _b in BITS:
    FULL |= _b
UNASSIGNED = [12, 14] + list(range(26, 32))
assert len(BITS) == 24 and FULL == (1 << 26) - 1 - (1 << 12) - (1 << 14)          # the 26-bit space: bits 0 .. 25 without 12 and 14

CALIPER = _abi.FAM_CALIPER
# kBehindIntensity of nyxhip_ctx.h: the families whose columns lie between the intensity block and GLCM -- the span a GLCM-holding feature
# launch zeroes.  tests/test_mask_lattice_cpu.py derives the same set from the column order.
BEHIND_INTENSITY = [_abi.FAM_ELLIPSE, _abi.FAM_EROSION, _abi.FAM_FRACTAL, _abi.FAM_FERET, _abi.FAM_MARTIN, _abi.FAM_NASSENSTEIN, _abi.FAM_CHORDS,
                    _abi.FAM_EULER, _abi.FAM_CIRCLES, _abi.FAM_GEODETIC, _abi.FAM_ROI_RADIUS]

# Columns whose arithmetic legitimately depends on the mask: {column name: reason, citing the code}.  Empty: every block is compared bit for
# bit across masks.
MASK_DEPENDENT = {}


def bits_of(mask):
    return [b for b in BITS if mask & b]


# ---- settings -------------------------------------------------------------------------------------------------------------------------
def settings_a():
    """Grey depth 8, four GLCM angles, the default Gabor bank: the GLCM columns of this order go through glcm_features_kernel."""
    return sc.settings(8)


def settings_b(n_angles=3, n_filters=5):
    """Grey depth 64, three GLCM angles, symmetric matrices, five Gabor filters: odd block widths."""
    s = sc.settings(64, na=n_angles)
    s.glcm_symmetric = 1
    s.gabor_n_filters = n_filters
    for i in range(4, n_filters):
        s.gabor_f0[i] = [4.0, 16.0, 32.0, 64.0][i % 4]
        s.gabor_theta[i] = np.pi * (2 * i + 1) / 32
    return s


SETTINGS = {"a": settings_a, "b": settings_b}


# ---- the batch ------------------------------------------------------------------------------------------------------------------------
CLASS_PX = (256, 4096, 16384, 32768)     # kClassPx / kClassSide of roi_kernel.h
CLASS_SIDE = (32, 64, 128, 256)
CONTOUR_PLANE_CAP = 16 * 1024            # bytes of the padded flag plane the contour kernel keeps in LDS in a batch with larger boxes
OUTLINE_BITS_LDS = 2048                  # kOutlineBitsLds of roi_outline.h


def roi_class(n, w, h, rng):
    """roi_class of roi_kernel.h without IBSI levels: 2 * size class + (1: the 16-bit counting tables are ruled out)."""
    side = max(w, h)
    k = 0
    while k < 4 and not (n <= CLASS_PX[k] and side <= CLASS_SIDE[k]):
        k += 1
    if k == 2 and rng >= 65536:
        k = 3
    return 2 * k + (0 if n < 65536 and rng < 16384 else 1)


def outline_bit_words(bw, bh):
    """outline_bit_words of roi_outline.h with the box pyramid (tests/test_deferred_lists_gpu.py)."""
    wd, rows = bw // 32 + 1, bh
    total, sd = wd * rows, outline_ref.ceil_pow2(max(bw, bh))
    while sd > 1:
        wd, rows = (wd + 1) // 2, (rows + 1) // 2
        total += wd * rows
        sd >>= 1
    return total


def listed(b):
    """{deferred list: rows of `b` for which its predicate (nyxhip_contour.hip, deferred_list.h) is true in this batch}."""
    w, h, mn = (np.asarray(a).astype(np.int64) for a in (b.bbox_w, b.bbox_h, b.min_inten))
    side = int(max(w.max(), h.max()))
    chords_lds = min(chords_cases.LDS_WORDS, chords_cases.plane_words(side, side))
    pred = {
        "CaliperWide": w > caliper_cases.LDS_COLS,
        "ChordsListed": (mn == 0) | (np.array([chords_cases.plane_words(a, c) for a, c in zip(w, h)]) > chords_lds),
        "ErosionListed": 2 * np.array([erosion_cases.plane_words(a, c) for a, c in zip(w, h)]) > erosion_cases.LDS_WORDS,
        "OutlineBitsBig": np.array([outline_bit_words(int(a), int(c)) for a, c in zip(w, h)]) > OUTLINE_BITS_LDS,
        "ContourPlaneBig": (w + 2) * (h + 2) > CONTOUR_PLANE_CAP,
    }
    return {k: list(np.flatnonzero(v)) for k, v in pred.items()}


def classes(b):
    n = np.diff(b.px_offset.astype(np.int64))
    rng = b.max_inten.astype(np.int64) - b.min_inten.astype(np.int64)
    return [roi_class(int(n[i]), int(b.bbox_w[i]), int(b.bbox_h[i]), int(rng[i])) for i in range(b.n_roi)]


def frame(h, w, t=1):
    m = np.ones((h, w), bool)
    m[t:-t, t:-t] = False
    return m


def _rois():
    rng = np.random.default_rng(26)
    one = np.zeros(30, np.uint32)
    one[17] = 77
    plate = np.kron(outline_cases.two_holes(), np.ones((4, 4), bool))                      # 36 x 60, two holes: an Euler number below 1
    named = [
        # degenerates
        ("one-pixel", sc.roi([0], [0], [9])),
        ("two-in-a-row", sc.box(2, 1, [3, 8])),
        ("anti-diagonal", sc.roi([1, 0], [0, 1], [5, 200])),
        ("constant-5x5", sc.box(5, 5, 1234)),
        ("one-non-zero", sc.box(6, 5, one)),                                               # zero-intensity pixels: listed for the chords
        # size classes 0 .. 4 (sc = class / 2); the odd classes: an intensity range that rules the 16-bit tables out
        ("sc0", synth.random_rois(12, seed=8, rmax=9, value_modes=(4096, 256))[2]),
        ("sc0-zeros", chords_cases.collision()),                                           # three zero-intensity pixels in a 6 x 6 block
        ("sc1", sc.eight_wave_companion()),                                                # 50 x 48
        ("sc1-odd", sc.wide_range_companion()),                                            # 25 x 25 disc, range beyond 16 bits
        ("sc1-holes", _mask_roi(plate, 949)),
        ("sc2", _mask_roi(disc(33), 33)),                                                  # 67 x 67: beyond a side of 64
        ("sc3", sc.box(130, 36, rng.integers(1, 4096, 130 * 36))),                         # beyond a side of 128
        ("sc3-odd", sc.box(30, 129, rng.integers(1, 200000, 30 * 129))),
        ("sc4-box", sc.box(258, 130, rng.integers(1, 4096, 258 * 130))),                   # beyond 32768 pixels and a side of 256: beyond LDS
        # thin shapes: large boxes, few pixels -- the deferred lists
        ("wide-line", _mask_roi(caliper_cases._wide(caliper_cases.LDS_COLS + 1)[0], 900)),  # CaliperWide, ChordsListed by its plane
        ("wide-diag", _mask_roi(caliper_cases._wide(caliper_cases.LDS_COLS + 9)[2], 901)),  # CaliperWide with a box 130 rows high
        ("frame", _mask_roi(frame(300, 900, 2), 930)),                                      # ErosionListed, OutlineBitsBig, ContourPlaneBig
        ("diagonal", _mask_roi(np.eye(180, dtype=bool)[:, ::-1], 960)),                    # ContourPlaneBig alone
        ("annulus", _mask_roi(disc(70) & ~np.pad(disc(69), 1), 961)),
    ]
    # distinct non-zero origins: the caliper, chords and circle families read them
    return [(k, dict(x=r["x"] + 11 + 977 * i, y=r["y"] + 7 + 3301 * i, inten=r["inten"])) for i, (k, r) in enumerate(named)]


_BATCH = None


def lattice_batch():
    """(HostBatch, names of its rows); checked to hold every kind of ROI the tests are about."""
    global _BATCH
    if _BATCH is None:
        named = _rois()
        b = _abi.batch_from_rois([r for _, r in named])
        keys = [k for k, _ in named]
        assert b.origin_x is not None and (b.origin_x > 0).all() and (b.origin_y > 0).all()
        assert len(set(zip(b.origin_x.tolist(), b.origin_y.tolist()))) == b.n_roi
        cl = classes(b)
        assert {c // 2 for c in cl} == {0, 1, 2, 3, 4}, cl                                 # every size class
        assert 3 in cl and 7 in cl and 2 in cl and 6 in cl, cl                             # both table widths in size classes 1 and 3
        assert cl[keys.index("sc4-box")] // 2 == 4
        L = listed(b)
        assert all(len(v) >= 1 for v in L.values()), L                                     # every deferred list has a member ...
        assert all(len(v) < b.n_roi for v in L.values()), L                                # ... and every LDS launch beside it has work
        assert (b.min_inten[L["ChordsListed"]] == 0).any() and (b.min_inten[L["ChordsListed"]] > 0).any()   # by zero pixels and by its plane
        n = np.diff(b.px_offset.astype(np.int64))
        assert sorted(n[:5]) == [1, 2, 2, 25, 30] and b.min_inten[3] == b.max_inten[3]
        _BATCH = (b, keys)
    return _BATCH


_LATE = None


def late_lane_batch():
    """(HostBatch, names of its rows): three thin frames whose boxes hold millions of cells -- the large classes' GLCM chain works on the
    box plane and takes long -- beside small ROIs; few pixels, so every family behind the intensity block is done quickly."""
    global _LATE
    if _LATE is None:
        named = [("frame-2500", _mask_roi(frame(2500, 2500, 2), 70)), ("sc3", sc.box(130, 36, np.random.default_rng(71).integers(1, 4096, 130 * 36))),
                 ("frame-2400", _mask_roi(frame(2400, 2600, 1), 72)), ("sc0", sc.box(5, 5, 1234)), ("frame-2000", _mask_roi(frame(2000, 3000, 3), 73)),
                 ("sc1", sc.eight_wave_companion())]
        rois = [dict(x=r["x"] + 5 + 3001 * i, y=r["y"] + 9 + 2003 * i, inten=r["inten"]) for i, (_, r) in enumerate(named)]
        b = _abi.batch_from_rois(rois)
        assert sum(c // 2 >= 3 for c in classes(b)) == 4 and int((b.bbox_w.astype(np.int64) * b.bbox_h).max()) >= 6_000_000
        _LATE = (b, [k for k, _ in named])
    return _LATE


def check_launch_report(rep, b):
    """The classes a call over `b` launched (nyxhip_launch_report of a call that holds a class-launched family; the batch's wide
    ranges make such a call take exact class lists): the restated class rule, ROI for ROI.  Size classes 3 and 4 of either table
    width run as one launch group, reported under the largest class among them."""
    def groups(pairs):
        out = {}
        for c, n in pairs:
            k = c if c < 6 else "large"
            out[k] = out.get(k, 0) + n
        return out
    want = groups((c, 1) for c in classes(b))
    got = groups((r["class"], r["rois"]) for r in rep if r["class"] >= 0 and r["rois"] > 0)
    assert got == want and want["large"] >= 2 and len(want) >= 5, (want, rep)
    return got


def tile_subset(b, keys, size=256):
    """The ROIs of the batch whose boxes fit one size x size tile, drawn into it by shelves (a pixel apart) -> (intensity tile, label tile,
    rows of `b` in label order).  Labels ascend with the row, so the tile path returns the rows in batch order."""
    it = np.zeros((size, size), np.uint32)
    lab = np.zeros((size, size), np.uint32)
    x0 = y0 = shelf = 0
    rows = []
    off = b.px_offset.astype(np.int64)
    order = sorted(range(b.n_roi), key=lambda r: -int(b.bbox_h[r]))
    placed = {}
    for r in order:
        w, h = int(b.bbox_w[r]), int(b.bbox_h[r])
        if w > 140 or h > 140:
            continue
        if x0 + w > size:
            x0, y0, shelf = 0, y0 + shelf + 1, 0
        if y0 + h > size:
            continue
        placed[r] = (x0, y0)
        x0 += w + 1
        shelf = max(shelf, h)
    for r in sorted(placed):
        px, py = placed[r]
        x, y = b.x[off[r]:off[r + 1]].astype(np.int64) + px, b.y[off[r]:off[r + 1]].astype(np.int64) + py
        assert (lab[y, x] == 0).all()
        lab[y, x] = r + 1
        it[y, x] = b.inten[off[r]:off[r + 1]]
        rows.append(r)
    assert len(rows) >= 12 and {keys[r] for r in rows} >= {"one-pixel", "one-non-zero", "sc1-odd", "sc2", "sc3", "sc3-odd"}, [keys[r] for r in rows]
    return it, lab, rows


# ---- the masks ------------------------------------------------------------------------------------------------------------------------
def _subsets(parts):
    for k in range(len(parts) + 1):
        for c in itertools.combinations(parts, k):
            m = 0
            for p in c:
                m |= p
            yield m


def masks():
    """{group: list of masks}, deterministic."""
    INT, GLCM = _abi.FAM_INTENSITY, _abi.FAM_GLCM
    g = {"singles": list(BITS), "full": [FULL], "leave_one_out": [FULL & ~b for b in BITS]}
    g["glcm_span"] = [m for b in BEHIND_INTENSITY for m in (b | GLCM, b | INT | GLCM, b | INT)]
    inter = [_abi.FAM_RADIAL | m for m in _subsets([_abi.FAM_GABOR, _abi.FAM_ZERNIKE, _abi.FAM_NGTDM, _abi.FAM_SMOMS])]
    parts = [_abi.FAM_FERET, _abi.FAM_MARTIN, _abi.FAM_NASSENSTEIN, _abi.FAM_CHORDS, _abi.FAM_CIRCLES, _abi.FAM_GEODETIC, _abi.FAM_ELLIPSE | _abi.FAM_EROSION]
    for f in (_abi.FAM_FRACTAL, _abi.FAM_EULER, _abi.FAM_ROI_RADIUS):
        inter += [f | m for m in _subsets(parts)]
    g["interleave"] = list(dict.fromkeys(inter))
    rng = np.random.default_rng(26)
    rnd = []
    while len(rnd) < 48:
        p = (0.2, 0.5, 0.8)[int(rng.integers(0, 3))]
        m = 0
        for b in BITS:
            if rng.random() < p:
                m |= b
        if m and m not in rnd:
            rnd.append(m)
    g["random"] = rnd
    return g
