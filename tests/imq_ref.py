"""A numpy restatement of the reference's FocusScoreFeature (features/focus_score.cpp:188-282) and SaturationFeature
(features/saturation.cpp:74-95) over the ROI's dense plane -- test infrastructure: the generator of tests/golden/imq refuses to store a
recording this file disagrees with, and the side-1 boxes, which the reference cannot be given, are checked against it alone."""
import numpy as np

NAMES = ["FOCUS_SCORE", "LOCAL_FOCUS_SCORE", "MAX_SATURATION", "MIN_SATURATION"]
FOCUS = [0, 1]
SATURATION = [2, 3]


def plane(b, r):
    """The dense plane of ROI r of a host batch: [h, w] uint32, the cloud's intensities, 0 elsewhere (LR::aux_image_matrix)."""
    o, e = int(b.px_offset[r]), int(b.px_offset[r + 1])
    P = np.zeros((int(b.bbox_h[r]), int(b.bbox_w[r])), np.uint32)
    P[b.y[o:e].astype(np.int64), b.x[o:e].astype(np.int64)] = b.inten[o:e]
    return P


def laplacian(P):
    """L = up + down + left + right - 4 * centre with zeros outside the plane, in fp64 (every value is an exact integer)."""
    Z = np.zeros((P.shape[0] + 2, P.shape[1] + 2))
    Z[1:-1, 1:-1] = P
    return Z[:-2, 1:-1] + Z[2:, 1:-1] + Z[1:-1, :-2] + Z[1:-1, 2:] - 4.0 * Z[1:-1, 1:-1]


def variance(L):
    """Population variance, the reference's two passes: mean = sum / n, then the mean squared deviation."""
    v = L.ravel()
    mean = v.sum() / v.size
    return float(((v - mean) ** 2).sum() / v.size)


def tile_origins(h, w):
    """The (y0, x0) the reference's loop visits: y0 = 0, M, 2M, .. while y0 < h - M, x0 likewise, M = h // 2, N = w // 2."""
    M, N = h // 2, w // 2
    if M == 0 or N == 0:
        raise ValueError("a side of 1: the reference's loop does not end")
    return [(y0, x0) for y0 in range(0, h - M, M) for x0 in range(0, w - N, N)]


def local_focus(P):
    h, w = P.shape
    M, N = h // 2, w // 2
    total = 0.0
    for y0, x0 in tile_origins(h, w):
        total += variance(laplacian(P[y0:y0 + M, x0:x0 + N]))
    return total / 4.0


def saturation(P):
    """(MAX_SATURATION, MIN_SATURATION): if (pix == max) .. else if (pix == min), each count divided by the number of cells."""
    mx, mn = int(P.max()), int(P.min())
    n_max = int((P == mx).sum())
    n_min = 0 if mn == mx else int((P == mn).sum())
    return float(np.float64(n_max) / np.float64(P.size)), float(np.float64(n_min) / np.float64(P.size))


def row_of_plane(P, soft_nan):
    if P.size == 0:
        return [soft_nan] * 4
    h, w = P.shape
    loc = soft_nan if (h < 2 or w < 2) else local_focus(P)
    mx, mn = saturation(P)
    return [variance(laplacian(P)), loc, mx, mn]


def table(b, s):
    """[n_roi x 4] of a host batch under settings s."""
    out = np.zeros((b.n_roi, 4))
    for r in range(b.n_roi):
        if int(b.px_offset[r + 1]) == int(b.px_offset[r]) or int(b.bbox_w[r]) * int(b.bbox_h[r]) == 0:
            out[r] = s.soft_nan
        else:
            out[r] = row_of_plane(plane(b, r), float(s.soft_nan))
    return out


def same_bits(a, w):
    a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
    return (a.view(np.uint64) == w.view(np.uint64)) | (np.isnan(a) & np.isnan(w))


def rel_diff(a, w):
    """|a - w| / |w|, 0 where the bits agree; where w is 0 any difference is infinite (an exact 0 is asked for)."""
    a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(a - w) / np.abs(w)
    return np.where(same_bits(a, w) | (a == w), 0.0, np.where(w == 0, np.inf, d))
