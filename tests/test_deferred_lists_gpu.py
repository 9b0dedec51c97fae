"""The deferred lists of nyxus_amd/csrc/nyxhip_contour.hip (deferred_list.h) with more than one chunk: one test per owner -- caliper,
chords, erosion, outline, the contour chain.  Each batch mixes small ROIs (served from LDS) with K listed ROIs (served from the
per-workgroup global workspace), K chosen with the stride the launcher computes -- restated here from the constants of the case
modules -- so that the K workspaces take at least 3 MiB and that K is no multiple of the chunk a 1 MiB budget
(NYXHIP_LARGE_BUDGET_MB=1) allows: several full chunks and a shorter last one.  Asserted per owner:
  (a) the rows are those of the family's CPU restatement: bit for bit, except FRACT_DIM_BOXCOUNT / FRACT_DIM_PERIMETER (sums of
      logarithms: the device's log is not the host's libm; the bounds of tests/test_outline_gpu.py) and RADIAL_CV (parity.REL_TOL, as
      in tests/test_radial_gpu.py);
  (b) the rows under the 1 MiB budget are the rows without it, bit for bit, NaNs matching NaNs;
  (c) the rows of the listed ROIs alone are their rows in the mixed batch.
The listed shapes are thin (lines, diagonals, frames): the workspaces grow with the boxes, the CPU restatements with the pixels."""
import numpy as np
import pytest

from nyxus_amd import _abi, _lib
from tests import caliper_cases, caliper_ref, chords_cases, chords_ref, circle_ref, erosion_cases, erosion_ref, outline_cases, outline_ref, parity
from tests import radial_cases, radial_ref, synth
from tests.radial_cases import _mask_roi, disc

pytestmark = pytest.mark.gpu

BUDGET = 1 << 20                     # NYXHIP_LARGE_BUDGET_MB=1
CONTOUR_PLANE_CAP = 16 * 1024        # bytes of the padded flag plane (w + 2)(h + 2) the contour kernel keeps in LDS in a batch with larger boxes
OUTLINE_BITS_LDS = 2048              # kOutlineBitsLds of roi_outline.h
CALIPER_BYTES_PER_COL = 24           # kCaliperBytesPerCol of roi_caliper.h


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def r64(v):
    return (int(v) + 63) & ~63


def plan(k, stride):
    """The chunk of k listed ROIs of `stride` bytes each under BUDGET (deferred_chunk): checked to give full chunks and a shorter last one."""
    chunk = max(1, min(k, BUDGET // stride))
    assert k * stride >= 3 << 20 and chunk >= 2 and k % chunk != 0 and k > 2 * chunk, (k, stride, chunk)
    return chunk


def mixed_batch(small, listed):
    """The listed ROIs spread among the small ones -> (batch, rows of the listed ROIs)."""
    rois, at = [], []
    for i in range(max(len(small), len(listed))):
        if i < len(small):
            rois.append(small[i])
        if i < len(listed):
            at.append(len(rois))
            rois.append(listed[i])
    return rois, at


def run(ctx, monkeypatch, small, listed, mask, s):
    """Rows of the mixed batch after (b) and (c) have been checked on them."""
    rois, at = mixed_batch(small, listed)
    b = _abi.batch_from_rois(rois)
    got = ctx.featurize_host(b, mask, s)
    # The context's device table is reused from call to call and an ROI no launch serves keeps what the table held: the same ROIs
    # one row further leave every row with another ROI's values
    shifted = ctx.featurize_host(_abi.batch_from_rois(rois[1:] + rois[:1]), mask, s)
    assert not same(shifted[at], got[at])
    monkeypatch.setenv("NYXHIP_LARGE_BUDGET_MB", "1")
    chunked = ctx.featurize_host(b, mask, s)
    monkeypatch.delenv("NYXHIP_LARGE_BUDGET_MB")
    assert same(chunked, got), np.argwhere(~((chunked == got) | (np.isnan(chunked) & np.isnan(got))))[:8]
    alone = ctx.featurize_host(_abi.batch_from_rois(listed), mask, s)
    assert same(alone, got[at]), np.argwhere(~((alone == got[at]) | (np.isnan(alone) & np.isnan(got[at]))))[:8]
    return b, at, got


def _place(rois, dx=11, dy=7):
    return [dict(r, x=r["x"] + dx * i, y=r["y"] + dy * i) for i, r in enumerate(rois)]


def frame(h, w, t=1):
    m = np.ones((h, w), bool)
    m[t:-t, t:-t] = False
    return m


def diagonal(n, flip=False):
    m = np.eye(n, dtype=bool)
    return m[:, ::-1] if flip else m


def ell(h, w):
    m = np.zeros((h, w), bool)
    m[:, 0] = m[-1, :] = True
    return m


def annulus(r):
    """A circle line one to two pixels thick: the rim of radial_cases.disc(r)."""
    return disc(r) & ~np.pad(disc(r - 1), 1)


# ---- caliper: ROIs wider than the LDS column table; tables of kCaliperBytesPerCol bytes per column of the widest box, rounded up to 32 columns
def caliper_rois():
    W = caliper_cases._wide
    ms = [W(20000)[0], W(20000)[2], W(20000)[1], W(9000)[0], W(9001)[2], W(5000)[1], W(caliper_cases.LDS_COLS + 1)[0]]
    return caliper_cases.shapes()[:6], _place([_mask_roi(m, 900 + i) for i, m in enumerate(ms)])


def test_caliper_list_in_several_chunks(hip_ctx, monkeypatch):
    small, listed = caliper_rois()
    b, at, got = run(hip_ctx, monkeypatch, small, listed, _abi.FAM_FERET | _abi.FAM_MARTIN | _abi.FAM_NASSENSTEIN, _abi.default_settings(64))
    is_listed = np.asarray(b.bbox_w) > caliper_cases.LDS_COLS
    assert list(np.flatnonzero(is_listed)) == at
    side = int(max(np.asarray(b.bbox_w).max(), np.asarray(b.bbox_h).max()))
    stride = CALIPER_BYTES_PER_COL * ((min(side, 65535) + 31) & ~31)
    print("caliper: listed", len(at), "stride", stride, "chunk", plan(len(at), stride))
    want = caliper_ref.table(b)
    assert np.isfinite(want).all()
    assert same(got, want), np.argwhere(got != want)[:8]


# ---- chords: ROIs whose rotated bit plane exceeds LDS, or with zero-intensity pixels; a bit plane of the largest chords_plane_words among
# them and a word per cell of the largest chords_plane_side squared among those with zero-intensity pixels, each rounded up to 64 words
def chords_rois():
    ms = [m for n in (1500, 1400, 1300, 1200) for m in chords_cases._thin(n)]
    listed = [_mask_roi(m, 910 + i) for i, m in enumerate(ms)] + [chords_cases.collision()]   # (the last one: three zero-intensity pixels)
    return chords_cases.shapes()[:6], _place(listed)


def test_chords_list_in_several_chunks(hip_ctx, monkeypatch):
    small, listed = chords_rois()
    s = _abi.default_settings(64)
    b, at, got = run(hip_ctx, monkeypatch, small, listed, _abi.FAM_CHORDS, s)
    w, h, mn = (np.asarray(a).astype(np.int64) for a in (b.bbox_w, b.bbox_h, b.min_inten))
    words = np.array([chords_cases.plane_words(a, c) for a, c in zip(w, h)])
    sides = np.array([chords_cases.plane_side(a, c) for a, c in zip(w, h)])
    lds_words = min(chords_cases.LDS_WORDS, chords_cases.plane_words(max(w.max(), h.max()), max(w.max(), h.max())))
    is_listed = (mn == 0) | (words > lds_words)
    assert list(np.flatnonzero(is_listed)) == at and (mn[at] == 0).sum() == 1
    stride = 4 * (r64(words[is_listed].max()) + r64(int(sides[is_listed & (mn == 0)].max()) ** 2))
    print("chords: listed", len(at), "stride", stride, "chunk", plan(len(at), stride))
    want = chords_ref.table(b)
    assert same(got, want), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:8]


# ---- erosion: ROIs whose two bit planes exceed LDS; two planes of the largest erosion_plane_words among them, rounded up to 64 words
def erosion_rois():
    boxes = [(600, 3000, 4), (300, 2000, 9), (900, 1000, 6), (640, 640, 12), (601, 2999, 1), (4000, 33, 7), (599, 3000, 15)]    # (rows, columns, thickness)
    listed = [_mask_roi(frame(h, w, t), 930 + i) for i, (h, w, t) in enumerate(boxes)]
    return erosion_cases.shapes()[:6], listed


def test_erosion_list_in_several_chunks(hip_ctx, monkeypatch):
    small, listed = erosion_rois()
    b, at, got = run(hip_ctx, monkeypatch, small, listed, _abi.FAM_EROSION, _abi.default_settings(64))
    words = np.array([erosion_cases.plane_words(w, h) for w, h in zip(b.bbox_w, b.bbox_h)])
    is_listed = 2 * words > erosion_cases.LDS_WORDS
    assert list(np.flatnonzero(is_listed)) == at
    stride = 4 * r64(2 * words[is_listed].max())
    print("erosion: listed", len(at), "stride", stride, "chunk", plan(len(at), stride))
    want = erosion_ref.table(b)[:, 6:]
    assert len(set(want[at, 0])) >= 5 and (want[at, 0] > 0).sum() >= 6       # frames of several thicknesses: as many pass counts
    assert same(got, want), np.argwhere(got != want)[:8]


# ---- outline: ROIs whose bit planes (mask + box pyramid) exceed LDS; the smaller of the bound over the batch extrema and the planes of a
# square of the largest side, rounded up to 64 words
def outline_rois():
    ms = [diagonal(1224), ell(1000, 1500), diagonal(1200, flip=True), frame(700, 800), diagonal(1100), ell(1225, 1224), diagonal(1000, flip=True),
          frame(500, 900, 2), annulus(200)]
    plate = np.kron(outline_cases.two_holes(), np.ones((4, 4), bool))        # 36 x 60: within LDS
    return synth.random_rois(5, seed=78, rmax=25) + [_mask_roi(plate, 949)], [_mask_roi(m, 940 + i) for i, m in enumerate(ms)]


def test_outline_list_in_several_chunks(hip_ctx, monkeypatch):
    small, listed = outline_rois()
    s = _abi.default_settings(64)
    b, at, got = run(hip_ctx, monkeypatch, small, listed, _abi.FAM_FRACTAL | _abi.FAM_EULER | _abi.FAM_ROI_RADIUS, s)
    w, h = np.asarray(b.bbox_w).astype(np.int64), np.asarray(b.bbox_h).astype(np.int64)

    def bit_words(bw, bh):                                                   # outline_bit_words of roi_outline.h, with the pyramid
        wd, rows = bw // 32 + 1, bh
        total, sd = wd * rows, outline_ref.ceil_pow2(max(bw, bh))
        while sd > 1:
            wd, rows = (wd + 1) // 2, (rows + 1) // 2
            total += wd * rows
            sd >>= 1
        return total
    max_area, max_side = int((w * h).max()), int(max(w.max(), h.max()))
    bound = 2 * (max_area // 32 + max_side) + 2 * max_side + 64
    assert bound > OUTLINE_BITS_LDS
    is_listed = np.array([bit_words(int(a), int(c)) for a, c in zip(w, h)]) > OUTLINE_BITS_LDS
    assert list(np.flatnonzero(is_listed)) == at
    stride = 4 * r64(min(bound, bit_words(min(max_side, 65535), min(max_side, 65535))))
    print("outline: listed", len(at), "stride", stride, "chunk", plan(len(at), stride))
    want = outline_ref.outline_table(b)
    assert np.isfinite(want).all()                                           # no one-point contour: the reference defines every value
    bad = outline_cases.mismatches(got, want, parity.REL_TOL)
    assert not bad, "\n".join(bad[:10])
    assert same(got[:, 2:], want[:, 2:]), np.argwhere(got[:, 2:] != want[:, 2:])[:8]   # Euler number, radius mean / max / median: the same bits


# ---- the contour chain: ROIs whose padded flag plane exceeds the LDS plane; a plane of max_area + 4 max_side + 4 bytes, rounded up to 256
def contour_rois():
    ms = [annulus(340), diagonal(680), diagonal(660, flip=True), ell(600, 681), annulus(150), frame(300, 500), diagonal(500)]
    return synth.random_rois(6, seed=3, rmax=20), [_mask_roi(m, 960 + i) for i, m in enumerate(ms)]


def test_contour_list_in_several_chunks(hip_ctx, monkeypatch):
    small, listed = contour_rois()
    s = _abi.default_settings(64)
    mask = _abi.FAM_RADIAL | _abi.FAM_CIRCLES | _abi.FAM_GEODETIC | _abi.FAM_SMOMS | _abi.FAM_IMOMS
    b, at, got = run(hip_ctx, monkeypatch, small, listed, mask, s)
    w, h = np.asarray(b.bbox_w).astype(np.int64), np.asarray(b.bbox_h).astype(np.int64)
    is_listed = (w + 2) * (h + 2) > CONTOUR_PLANE_CAP
    assert list(np.flatnonzero(is_listed)) == at
    stride = (int((w * h).max()) + 4 * int(max(w.max(), h.max())) + 4 + 255) & ~255
    print("contour: listed", len(at), "stride", stride, "chunk", plan(len(at), stride))
    names = _lib.column_names(mask, s)
    K = radial_ref.contours_of(b)
    want_r, D = radial_ref.radial_table(b, K, with_dst2=True)
    assert all(d is not None and d != 0 for d in D)                          # every radial centre is defined in the reference
    got_r = got[:, radial_ref.split_columns(names)]
    bad = parity.compare_tables(got_r, want_r, radial_ref.NAMES, exact=radial_ref.EXACT)
    assert not bad, bad[:10]
    exact = [i for i, n in enumerate(radial_ref.NAMES) if n in radial_ref.EXACT]
    assert same(got_r[:, exact], want_r[:, exact])
    want_c = circle_ref.table(b, K)[:, :5]
    got_c = got[:, [names.index(n) for n in circle_ref.NAMES]]
    assert same(got_c, want_c), [(r, circle_ref.NAMES[c], got_c[r, c], want_c[r, c]) for r, c in np.argwhere(got_c != want_c)[:8]]
