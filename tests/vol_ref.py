"""A NumPy restatement of the reference's two volumetric classes on a HostBatch3D -- the CPU reference of the volume tests and of
tools/vol_fuzz.py.  tests/golden/vol/make_vol_golden.py asserts it against the reference's own classes on every recorded case.

  D3_GLCM_feature (features/3d_glcm.cpp): the dense box of level indices (features/texture_feature.h:52-76), per direction of shifts[]
      the EXACT integer co-occurrence matrix (:326-371), then the closing formulas in fp64 with the reference's float32 fast_log10
      (helpers.h:283-330), and the _AVE values in the order of std::reduce (texture_feature.h:121-130).
  D3_VoxelIntensityFeatures (features/3d_intensity.cpp:45-183): a voxel cloud is a pixel cloud to every first-order formula, and the
      text is intensity.cpp's but for 3COVERED_IMAGE_INTENSITY_RANGE without a slide (1, not 0): the block is the C restatement of the
      2-D class (the project's test-only checker, run on the cloud as a one-row ROI) with that one column set.

Where the reference is undefined (vol_cases.rule_excluded) the values are this package's defined ones: an ROI without voxels is a row
of soft_nan; a flat ROI under radiomics binning has level 0 everywhere, so every direction is blank.
"""
from __future__ import annotations

import numpy as np

from nyxus_amd import _abi
from tests.vol_cases import N_ANG, N_AVE, N_COL, N_DIR, N_INT, SHIFTS

EPS = 0.000000001            # 3d_glcm.h:252
LOG10_2 = 0.30102999566      # 3d_glcm.h:244

# 2-D slot order of the 30 angled codes (the closing below fills it), and the Feature3D order: ACOR and ASM change places
_ANG_2D = ["ASM", "ACOR", "CLUPROM", "CLUSHADE", "CLUTEND", "CONTRAST", "CORRELATION", "DIFAVE", "DIFENTRO", "DIFVAR", "DIS", "ENERGY", "ENTROPY", "HOM1",
           "HOM2", "ID", "IDN", "IDM", "IDMN", "INFOMEAS1", "INFOMEAS2", "IV", "JAVE", "JE", "JMAX", "JVAR", "SUMAVERAGE", "SUMENTROPY", "SUMVARIANCE",
           "VARIANCE"]
ANG_3D = ["ACOR", "ASM"] + _ANG_2D[2:]
AVE_3D = ["ASM", "ACOR", "CLUPROM", "CLUSHADE", "CLUTEND", "CONTRAST", "CORRELATION", "DIFAVE", "DIFENTRO", "DIFVAR", "DIS", "ENERGY", "ENTROPY", "HOM1",
          "ID", "IDN", "IDM", "IDMN", "IV", "JAVE", "JE", "INFOMEAS1", "INFOMEAS2", "VARIANCE", "JMAX", "JVAR", "SUMAVERAGE", "SUMENTROPY", "SUMVARIANCE"]


def fast_log10(x):
    """helpers.h:283-330 on an array: float32 quadratic fit of log2 on the significand + the exponent, times 0.30102999566."""
    xf = np.asarray(x, np.float64).astype(np.float32)
    ui = xf.view(np.uint32)
    ex = ((ui & np.uint32(0x7F800000)) >> np.uint32(23)).astype(np.float32)
    gt = (ui & np.uint32(0x00400000)) != 0
    sig = np.where(gt, ((ui & np.uint32(0x007FFFFF)) | np.uint32(0x3F000000)).view(np.float32), ((ui & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(np.float32))
    fexp = np.where(gt, ex - np.float32(126.0), ex - np.float32(127.0)).astype(np.float32)
    sig = (sig - np.float32(1.0)).astype(np.float32)
    a, b = np.float32(-.6296735), np.float32(1.466967)
    lg2 = ((fexp + (a * sig).astype(np.float32) * sig).astype(np.float32) + (b * sig).astype(np.float32)).astype(np.float32)
    return lg2.astype(np.float64) * 0.30102999566


def _flog2(x):
    return fast_log10(x) / LOG10_2


def bin_levels(v: np.ndarray, vmin: int, vmax: int, grey_info: int) -> np.ndarray:
    """texture_feature.h:52-76 on the voxel values (uint32): radiomics (< 0), matlab (> 0), identity (0)."""
    v = v.astype(np.uint32)
    if grey_info < 0:
        n = -grey_info
        if vmax == vmin:
            return np.zeros(len(v), np.int64)              # undefined in the reference; defined here (module docstring)
        binw = float(vmax - vmin) / float(n)
        y = ((v.astype(np.int64) - vmin).astype(np.float64) / binw + 1).astype(np.int64)
        y = np.minimum(y, n)
        return np.where(v == 0, 0, y)
    if grey_info > 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            slope = np.float64(grey_info) / (np.float64(vmax) - 0.0)
            t = np.floor(slope * v.astype(np.float64) + 1.0)
        y = np.where(np.isfinite(t), np.minimum(t, 4.0e9), 4.0e9).astype(np.int64)
        y = np.clip(y, 1, grey_info)
        return np.where(v == 0, 1, y)
    return v.astype(np.int64)


def cooc(D: np.ndarray, shift, offset: int, grey_info: int, symmetric: bool):
    """(exact int64 matrix P[centre index, neighbour index], level values I) of one direction; D[z, y, x] holds levels."""
    d, h, w = D.shape
    if grey_info < 0:
        I = np.unique(D[D > 0])
    elif grey_info > 0:
        I = np.arange(1, grey_info + 1)
    else:
        I = np.arange(1, int(D.max()) + 1) if D.size else np.zeros(0, np.int64)
    Ng = len(I)
    P = np.zeros((Ng, Ng), np.int64)
    dx, dy, dz = (c * offset for c in shift)

    def span(n, dlt):       # centre coordinates c with 0 <= c + dlt < n
        lo, hi = max(0, -dlt), min(n, n - dlt)
        return (lo, hi) if hi > lo else None
    sx, sy, sz = span(w, dx), span(h, dy), span(d, dz)
    if Ng == 0 or sx is None or sy is None or sz is None:
        return P, I
    b = D[sz[0]:sz[1], sy[0]:sy[1], sx[0]:sx[1]].ravel()
    a = D[sz[0] + dz:sz[1] + dz, sy[0] + dy:sy[1] + dy, sx[0] + dx:sx[1] + dx].ravel()
    keep = (a != 0) & (b != 0)
    a, b = a[keep], b[keep]
    if grey_info < 0:
        ia, ib = np.searchsorted(I, a), np.searchsorted(I, b)
    else:
        ia, ib = a - 1, b - 1
    P += np.bincount(ib * Ng + ia, minlength=Ng * Ng).reshape(Ng, Ng)
    if symmetric or grey_info <= 0:
        P += np.bincount(ia * Ng + ib, minlength=Ng * Ng).reshape(Ng, Ng)
    return P, I


def close(P: np.ndarray, I: np.ndarray, soft_nan: float) -> dict:
    """The 30 values of one direction from its integer matrix (3d_glcm.cpp:179-259, :379-1077).  P[r, c] is the reference's
    P_matrix.yx(r, c) = xy(c, r)."""
    sum_p = float(P.sum())
    if sum_p == 0:
        return {k: soft_nan for k in _ANG_2D}
    Ng = len(I)
    Iv = I.astype(np.float64)
    Pf = P.astype(np.float64)
    p = Pf / sum_p
    r, c = np.indices((Ng, Ng))
    ir, ic = Iv[r], Iv[c]
    with np.errstate(invalid="ignore", divide="ignore"):
        Pxpy = np.bincount((r + c).ravel(), weights=p.ravel(), minlength=2 * Ng)
        Pxmy = np.bincount(np.abs(r - c).ravel(), weights=p.ravel(), minlength=Ng)
        k2 = np.arange(2 * Ng)
        xs = np.minimum(k2, Ng - 1)
        ksum = np.where(k2 <= 2 * Ng - 2, Iv[xs] + Iv[np.clip(k2 - xs, 0, Ng - 1)], 0.0)
        k1 = np.arange(Ng)
        kdiff = np.abs(Iv[Ng - 1] - Iv[Ng - 1 - k1])
        px = p.sum(axis=0)                                  # px[i] = sum_j xy(i, j) / sum_p: column sums
        py = p.sum(axis=1)
        brm = float((px * Iv).sum())
        f = {}
        f["ASM"] = float((p * p).sum())
        f["ENERGY"] = f["ASM"]
        f["CONTRAST"] = float((Pf * (ir - ic) ** 2).sum() / sum_p)
        mr = float((Pf * ir).sum() / sum_p)
        mc = float((Pf * ic).sum() / sum_p)
        sr = np.sqrt((p * (ir - mr) ** 2).sum())
        sc = np.sqrt((p * (ic - mc) ** 2).sum())
        f["CORRELATION"] = float(((ir - mr) * (ic - mc) * p).sum() / (sr * sc))
        f["HOM1"] = float((p / (1.0 + np.abs(r - c))).sum())
        mean = float((Pf.sum(axis=1) * Iv).sum() / sum_p)
        f["VARIANCE"] = float((((ir - mean) ** 2) * Pf).sum() / sum_p)
        f["IDM"] = float((Pxmy / (1 + k1 * k1)).sum())
        f["SUMAVERAGE"] = float((ksum * Pxpy).sum())
        f["SUMENTROPY"] = float(-(Pxpy * _flog2(Pxpy + EPS)).sum())
        ent = float((p * _flog2(p + EPS)).sum())
        f["ENTROPY"] = -ent
        f["JE"] = -ent
        davg = float((kdiff * Pxmy).sum())
        f["DIFAVE"] = davg
        f["DIFVAR"] = float((Ng * ((k1 - davg) ** 2) * Pxmy).sum() / Ng)
        nz = Pxmy != 0
        f["DIFENTRO"] = float(-(Pxmy[nz] * _flog2(Pxmy[nz] + EPS)).sum())
        pp = px[c] * py[r]                                  # px[i] py[j] at xy(i, j) = P[j, i]
        lpp = _flog2(pp + EPS)
        hxy1 = float((p * lpp).sum())
        hxy2 = float((pp * lpp).sum())
        hx = float((px * _flog2(px + EPS)).sum())
        f["INFOMEAS1"] = float(np.float64(ent - hxy1) / np.float64(hx))
        f["INFOMEAS2"] = float(np.sqrt(np.abs(1 - np.exp(-2 * (-hxy2 + ent)))))
        f["ACOR"] = float((Pf * ir * ic).sum() / sum_p)
        m = ir + ic - brm - brm
        f["CLUPROM"] = float((m ** 4 * p).sum())
        f["CLUSHADE"] = float((m ** 3 * p).sum())
        f["CLUTEND"] = float((m ** 2 * p).sum())
        f["SUMVARIANCE"] = f["CLUTEND"]
        f["DIS"] = float((np.abs(r - c) * p).sum())
        f["HOM2"] = float((p / (1.0 + (r - c) ** 2)).sum())
        f["IDMN"] = float((Pxmy / (1.0 + (k1 * k1) / float(Ng * Ng))).sum())
        f["ID"] = float((Pxmy / (1.0 + k1)).sum())
        f["IDN"] = float((Pxmy / (1.0 + k1 / float(Ng))).sum())
        f["IV"] = float((Pxmy[1:] / (kdiff[1:] ** 2)).sum())
        jave = float((Pf * ir).sum() / sum_p)
        f["JAVE"] = jave
        f["JMAX"] = float(p.max())
        f["JVAR"] = float((((c + 1) - jave) ** 2 * p).sum())   # x of xy(x, y) is the column
    return f


def reduce13(v) -> float:
    """std::reduce of libstdc++ over 13 values (four at a time, then the rest), divided by 13."""
    init = 0.0
    for q in range(0, 12, 4):
        init = init + ((v[q] + v[q + 1]) + (v[q + 2] + v[q + 3]))
    init = init + v[12]
    return init / 13.0


def glcm_rows(b: _abi.HostBatch3D, s: _abi.Settings) -> np.ndarray:
    out = np.zeros((b.n_roi, N_ANG * N_DIR + N_AVE))
    g = 0 if s.ibsi else int(s.glcm_grey_depth)
    off = b.px_offset.astype(np.int64)
    for r in range(b.n_roi):
        sl = slice(off[r], off[r + 1])
        n = off[r + 1] - off[r]
        if n == 0:
            out[r] = s.soft_nan
            continue
        w, h, d = int(b.bbox_w[r]), int(b.bbox_h[r]), int(b.bbox_d[r])
        bg = bin_levels(np.zeros(1, np.uint32), int(b.min_inten[r]), int(b.max_inten[r]), g)[0]
        D = np.full((d, h, w), bg, np.int64)
        D[b.z[sl], b.y[sl], b.x[sl]] = bin_levels(b.inten[sl], int(b.min_inten[r]), int(b.max_inten[r]), g)
        vals = np.zeros((N_DIR, N_ANG))
        for k, sh in enumerate(SHIFTS):
            P, I = cooc(D, sh, int(s.glcm_offset), g, bool(s.glcm_symmetric))
            f = close(P, I, s.soft_nan)
            vals[k] = [f[c] for c in ANG_3D]
        out[r, :N_ANG * N_DIR] = vals.T.ravel()
        out[r, N_ANG * N_DIR:] = [reduce13(vals[:, ANG_3D.index(c)]) for c in AVE_3D]
    return out


def intensity_rows(b: _abi.HostBatch3D, s: _abi.Settings) -> np.ndarray:
    from oracle import pyoracle as po
    out = np.zeros((b.n_roi, N_INT))
    off = b.px_offset.astype(np.int64)
    live = [r for r in range(b.n_roi) if off[r + 1] > off[r]]
    out[[r for r in range(b.n_roi) if off[r + 1] == off[r]]] = s.soft_nan
    # the checker's ROIs have 16-bit coordinates: a cloud becomes rows of 32768 pixels
    rois = []
    for r in live:
        n = int(off[r + 1] - off[r])
        i = np.arange(n)
        d = {"x": i % 32768, "y": i // 32768, "inten": b.inten[off[r]:off[r + 1]], "min": int(b.min_inten[r]), "max": int(b.max_inten[r])}
        if b.slide_min is not None:
            d["slide_min"], d["slide_max"] = float(b.slide_min[r]), float(b.slide_max[r])
        rois.append(d)
    if rois:
        T = po.oracle_featurize(_abi.batch_from_rois(rois), _abi.FAM_INTENSITY, s)
        if b.slide_min is None:
            T[:, 1] = 1.0                                   # 3d_intensity.cpp:64-65
        out[live] = T
    return out


def table(b: _abi.HostBatch3D, s: _abi.Settings, vmask: int = _abi.VFAM_ALL) -> np.ndarray:
    parts = []
    if vmask & _abi.VFAM_INTENSITY:
        parts.append(intensity_rows(b, s))
    if vmask & _abi.VFAM_GLCM:
        parts.append(glcm_rows(b, s))
    return np.hstack(parts)
