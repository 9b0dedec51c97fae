"""A NumPy restatement of the reference's D3_GLDZM_feature under the ruling of DESIGN.md 4.5m, on a HostBatch3D -- the CPU reference of
the volume distance-zone tests and of tools/voldzone_fuzz.py.  tests/golden/voldzone/make_voldzone_golden.py asserts it against the
reference's own class on every recorded case the reference is defined on.

THE RULING.  Semantics are those of the text of 3d_gldzm.cpp, quirks included, except that a cell of level 0 is treated in every binning
mode as the reference treats it in IBSI mode: it forms no zone and it is always a border.

Two steps, so that a test can disturb the first: `tables(...)` gives the EXACT integers of one ROI -- the distance map, the zones as rows
(level, metric, size) and the matrix [level][metric - 1]; `columns(...)` closes them in fp64 with the reference's formulas
(3d_gldzm.cpp:377-502).  `move_count` is the perturbation hook of tests/test_voldzone_cpu.py.  `dist2border_walk` transcribes the
reference's own per-cell walk (3d_gldzm.cpp:330-375) for the tests of `dist_map`.
"""
from __future__ import annotations

import numpy as np

from nyxus_amd import _abi
from tests.vol_ref import bin_levels
from tests.voltex_ref import cube

N_COL = 18
ROWS = _abi.VOLDZONE_MAX_LEVELS + 1
EPS = 2.2e-16                # 3d_gldzm.h:67
NAMES = ["SDE", "LDE", "LGLZE", "HGLZE", "SDLGLE", "SDHGLE", "LDLGLE", "LDHGLE", "GLNU", "GLNUN", "ZDNU", "ZDNUN", "ZP", "GLM", "GLV", "ZDM", "ZDV", "ZDE"]


def grey_info(s: _abi.Settings) -> int:
    return 0 if s.ibsi else int(s.grey_depth)              # 3d_gldzm.cpp:68-73: n_levels is never set


def binned(b: _abi.HostBatch3D, r: int, s: _abi.Settings) -> np.ndarray:
    V, n, vmin, vmax = cube(b, r)
    return bin_levels(V.ravel().astype(np.uint32), vmin, vmax, grey_info(s)).reshape(V.shape)


def dist2border_walk(D: np.ndarray, x: int, y: int, z: int) -> int:
    """3d_gldzm.cpp:330-375, line by line, on D[z, y, x]."""
    d, h, w = D.shape
    dl = dr = dt = db = 0
    for x0 in range(x - 1, -1, -1):
        if D[z, y, x0] == 0 or x0 == 0:
            dl = x - x0
            break
    for x0 in range(x + 1, w):
        if D[z, y, x0] == 0 or x0 == w - 1:
            dr = x0 - x
            break
    for y0 in range(y - 1, -1, -1):
        if D[z, y0, x] == 0 or y0 == 0:
            dt = y - y0
            break
    for y0 in range(y + 1, h):
        if D[z, y0, x] == 0 or y0 == h - 1:
            db = y0 - y
            break
    return max(1, min(dl + 1, dr + 1, dt + 1, db + 1))


def _axis_dist(zero: np.ndarray, axis: int) -> np.ndarray:
    """min over the two directions of `axis` of (distance to the nearest border strictly beyond the cell, + 1): a border is a level-0
    cell or the face cell of the axis; a cell on the face has 1 on that side."""
    n = zero.shape[axis]
    shape = [1, 1, 1]
    shape[axis] = n
    k = np.arange(n).reshape(shape)
    first = [slice(None)] * 3
    first[axis] = slice(0, 1)
    before = np.maximum.accumulate(np.where(zero, k, 0), axis=axis)              # the last level-0 position at or before (0: the face)
    before = np.concatenate([np.zeros_like(before[tuple(first)]), np.delete(before, n - 1, axis=axis)], axis=axis)   # strictly before
    flip = [slice(None)] * 3
    flip[axis] = slice(None, None, -1)
    after = np.minimum.accumulate(np.where(zero, k, n - 1)[tuple(flip)], axis=axis)[tuple(flip)]
    after = np.concatenate([np.delete(after, 0, axis=axis), np.full_like(after[tuple(first)], n - 1)], axis=axis)
    return np.minimum(k - before + 1, after - k + 1)


def dist_map(D: np.ndarray) -> np.ndarray:
    """dist2border of every cell of D[z, y, x]: its own z-plane only, along x and y.  Static: the reference's VISITED marks are non-zero."""
    zero = D == 0
    return np.minimum(_axis_dist(zero, 2), _axis_dist(zero, 1)).astype(np.int64)


def zones6(D: np.ndarray, dist: np.ndarray):
    """(level, metric, size) of every 6-connected component of equal non-zero level, in raster order of the first cell."""
    n = D.size
    idx = np.arange(n).reshape(D.shape)
    us, vs = [], []
    for ax in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        same = (D[tuple(a)] == D[tuple(b)]) & (D[tuple(a)] != 0)
        us.append(idx[tuple(a)][same])
        vs.append(idx[tuple(b)][same])
    u, v = np.concatenate(us), np.concatenate(vs)
    parent = np.arange(n)
    for _ in range(4 * 64):                                # hook to the smaller root, then shortcut; every round at least halves a chain
        pu, pv = parent[u], parent[v]
        if (pu == pv).all():
            break
        np.minimum.at(parent, np.maximum(pu, pv), np.minimum(pu, pv))
        while True:
            pp = parent[parent]
            if (pp == parent).all():
                break
            parent = pp
    else:
        raise AssertionError("component labelling did not converge")
    fg = D.ravel() != 0
    roots, inv, size = np.unique(parent[fg], return_inverse=True, return_counts=True)
    metric = np.full(len(roots), np.iinfo(np.int64).max)
    np.minimum.at(metric, inv, dist.ravel()[fg])
    return np.stack([D.ravel()[roots], metric, size], axis=1).astype(np.int64).reshape(-1, 3)


def tables(b: _abi.HostBatch3D, r: int, s: _abi.Settings) -> dict:
    """The exact integers of ROI r, or None for an ROI without voxels:
      "dist"     int64 [d, h, w]: the distance map
      "zones"    int64 [n, 3]: (level, metric, size) in raster order of the first cell
      "matrix"   int64 [ROWS, Nd]: zones of level i and metric j + 1
    and what the closing reads besides: the voxel count."""
    V, n, vmin, vmax = cube(b, r)
    if n == 0:
        return None
    T = {"flat": vmin == vmax, "shape": V.shape, "n": n}
    if T["flat"]:
        return T
    D = binned(b, r, s)
    T["levels"] = np.unique(D)
    T["dist"] = dist_map(D)
    if D.max() < ROWS:
        Z = zones6(D, T["dist"])
        T["zones"] = Z
        Nd = int(Z[:, 1].max()) if len(Z) else 0
        T["matrix"] = np.bincount(Z[:, 0] * Nd + Z[:, 1] - 1, minlength=ROWS * Nd).reshape(ROWS, Nd).astype(np.int64) if Nd else np.zeros((ROWS, 0), np.int64)
    return T


def move_count(T: dict, up: bool = True) -> dict:
    """A copy of T with ONE count of the matrix moved to the neighbouring distance (a zone whose metric is one larger or smaller).  None
    when the matrix has no count to move."""
    M = T["matrix"]
    if M.sum() == 0:
        return None
    i, j = np.unravel_index(int(np.argmax(M)), M.shape)
    j2 = j + 1 if (up or j == 0) else j - 1
    if j2 >= M.shape[1]:
        M = np.concatenate([M, np.zeros((M.shape[0], 1), np.int64)], axis=1)
    else:
        M = M.copy()
    M[i, j] -= 1
    M[i, j2] += 1
    U = dict(T)
    U["matrix"] = M
    return U


def close(M: np.ndarray, n_vox: int) -> list:
    """calc_row_and_column_sum_vectors and calc_features (3d_gldzm.cpp:377-502) on the matrix [level][metric - 1].  Rows of absent
    levels add exactly 0 to every sum, so all rows above level 0 stand in."""
    P = M[1:].astype(np.float64)
    g = np.arange(1, M.shape[0], dtype=np.float64)[:, None]
    d = np.arange(1, M.shape[1] + 1, dtype=np.float64)[None, :]
    Mx, Md = P.sum(axis=1), P.sum(axis=0)
    Ns = P.sum()
    gg, dd = g[:, 0], d[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        sde = (Md / dd / dd).sum() / Ns
        lde = (dd * dd * Md).sum() / Ns
        zdnu = (Md * Md).sum() / Ns
        zdnun = zdnu / Ns
        lglze = (Mx / (gg * gg)).sum() / Ns
        hglze = ((gg * gg) * Mx).sum() / Ns
        glnu = (Mx * Mx).sum() / Ns
        glnun = glnu / Ns
        sdlgle = (P / g / g / d / d).sum() / Ns
        sdhgle = (g * g * P / d / d).sum() / Ns
        ldlgle = (d * d * P / g / g).sum() / Ns
        ldhgle = (g * g * d * d * P).sum() / Ns
        glm = (g * P).sum() / Ns
        zdm = (d * P).sum() / Ns
        nz = P > 0                                         # an empty cell adds 0 * log2(EPS) = 0
        zde = -(P[nz] / Ns * np.log2(P[nz] / Ns + EPS)).sum()
        zp = Ns / float(n_vox)
        pn = P / Ns
        glv = (((g - glm) * (g - glm)) * pn)[nz].sum()
        zdv = (((d - zdm) * (d - zdm)) * pn)[nz].sum()
    return [sde, lde, lglze, hglze, sdlgle, sdhgle, ldlgle, ldhgle, glnu, glnun, zdnu, zdnun, zp, glm, glv, zdm, zdv, zde]


def columns(T: dict, s: _abi.Settings) -> np.ndarray:
    """The 18 columns from the integers of one ROI."""
    if T is None or T["flat"]:                             # no voxels; a flat ROI answers before it bins (3d_gldzm.cpp:509-533)
        return np.full(N_COL, float(s.soft_nan))
    if "matrix" not in T:
        return np.full(N_COL, np.nan)                      # (more levels than the table holds: the entry refuses the call)
    return np.array(close(T["matrix"], T["n"]))


def table(b: _abi.HostBatch3D, s: _abi.Settings) -> np.ndarray:
    return np.array([columns(tables(b, r, s), s) for r in range(b.n_roi)]).reshape(b.n_roi, N_COL)
