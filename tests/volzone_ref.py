"""A NumPy restatement of the reference's D3_GLRLM_feature and D3_GLSZM_feature on a HostBatch3D -- the CPU reference of the volume zone
tests and of tools/volzone_fuzz.py.  tests/golden/volzone/make_volzone_golden.py asserts it against the reference's own classes on every
recorded case.

Two steps, so that a test can disturb the first: `tables(...)` gives the EXACT integer matrices of one ROI -- per direction the run
matrix [level][length - 1], and the zones as rows (level, size, count) in matrix order; `columns(...)` closes them in fp64 with the
reference's formulas (3d_glrlm.cpp:224-259, :325-704; 3d_glszm.cpp:531-645, :667-884).  `move_count` is the perturbation hook of
tests/test_volzone_cpu.py.

Runs: every direction of shifts13 points forward in raster order, so gather_rl_zones yields the maximal runs of equal non-zero level along
the direction.  Zones: gather_size_zones is a complete depth-first search over 26 neighbours, so a zone is a 26-connected component of
equal level other than the background level (1 under matlab binning, else 0).

Where the reference is undefined (volzone_cases.rule_excluded) the values are this package's defined ones: an ROI without voxels is a row
of soft_nan, and the square of a run length or zone size j is double(j) * double(j) (the reference's int product overflows).
"""
from __future__ import annotations

import numpy as np

from nyxus_amd import _abi
from tests.vol_ref import LOG10_2, bin_levels, fast_log10, reduce13
from tests.voltex_ref import cube

N_DIR = 13
N_CODES = 16
N_GLRLM = N_CODES * N_DIR + N_CODES
N_GLSZM = 16
N_COL = N_GLRLM + N_GLSZM
ROWS = _abi.VOLZONE_MAX_LEVELS + 1
EPS = 2.2e-16                # 3d_glrlm.h:159, 3d_glszm.h:129
# shifts13[] of 3d_glrlm.cpp:17-32, fields (dz, dy, dx)
SHIFTS13 = [(1, 1, 1), (1, 1, 0), (1, 1, -1), (1, 0, 1), (1, 0, 0), (1, 0, -1), (1, -1, 1), (1, -1, 0), (1, -1, -1), (0, 1, 1), (0, 1, 0), (0, 1, -1), (0, 0, 1)]


def grey_info(s: _abi.Settings, t: _abi.VolZoneSettings):
    return (0 if s.ibsi else int(t.glrlm_grey_depth)), (0 if s.ibsi else int(t.glszm_grey_depth))


def _binned(V, vmin, vmax, g):
    return bin_levels(V.ravel().astype(np.uint32), vmin, vmax, g).reshape(V.shape)


def dir_len(sh, d, h, w) -> int:
    """the longest possible run of a direction: the smallest box side among its non-zero components"""
    return min(n for c, n in zip(sh, (d, h, w)) if c)


def runs(D: np.ndarray, sh):
    """(level, length) of every maximal run of equal non-zero level along sh = (dz, dy, dx) in D[z, y, x]."""
    d, h, w = D.shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    back = np.full(D.shape, max(d, h, w), np.int64)        # steps back to the face where the line enters the box
    for c, k, n in zip(sh, (z, y, x), (d, h, w)):
        if c > 0:
            back = np.minimum(back, k)
        elif c < 0:
            back = np.minimum(back, n - 1 - k)
    line = ((z - back * sh[0]) * h + (y - back * sh[1])) * w + (x - back * sh[2])
    order = np.lexsort((back.ravel(), line.ravel()))
    lv, ln = D.ravel()[order], line.ravel()[order]
    cut = np.flatnonzero((lv[1:] != lv[:-1]) | (ln[1:] != ln[:-1])) + 1
    start = np.concatenate([[0], cut])
    length = np.diff(np.concatenate([start, [len(lv)]]))
    keep = lv[start] != 0
    return lv[start][keep], length[keep]


def components(D: np.ndarray, zero_i: int):
    """(level, size) of every 26-connected component of equal level other than zero_i, in raster order of the first cell."""
    d, h, w = D.shape
    n = D.size
    idx = np.arange(n).reshape(D.shape)
    us, vs = [], []
    for dz in (0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) <= (0, 0, 0):
                    continue
                a = (slice(0, d - dz), slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx)))
                b = (slice(dz, d), slice(max(0, dy), h + min(0, dy)), slice(max(0, dx), w + min(0, dx)))
                same = (D[a] == D[b]) & (D[a] != zero_i)
                us.append(idx[a][same])
                vs.append(idx[b][same])
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
    fg = D.ravel() != zero_i
    roots, size = np.unique(parent[fg], return_counts=True)
    return D.ravel()[roots], size


def tables(b: _abi.HostBatch3D, r: int, s: _abi.Settings, t: _abi.VolZoneSettings) -> dict:
    """The exact integer matrices of ROI r, or None for an ROI without voxels.
      "glrlm"   list of 13 int64 arrays [ROWS][L_k]: runs of level i and length j + 1 along direction k
      "zones"   int64 array [n, 3]: (level, size, count), sorted by level, then size
    and what the closing reads besides: the voxel count, the distinct levels of either binned box."""
    V, n, vmin, vmax = cube(b, r)
    if n == 0:
        return None
    d, h, w = V.shape
    T = {"flat": vmin == vmax, "shape": (d, h, w), "n": n}
    if T["flat"]:
        return T
    g_rl, g_sz = grey_info(s, t)
    D = _binned(V, vmin, vmax, g_rl)
    T["rl_levels"] = np.unique(D)
    if D.max() < ROWS:
        T["glrlm"] = []
        for sh in SHIFTS13:
            lv, ln = runs(D, sh)
            L = dir_len(sh, d, h, w)
            T["glrlm"].append(np.bincount(lv * L + ln - 1, minlength=ROWS * L).reshape(ROWS, L).astype(np.int64))
    D = _binned(V, vmin, vmax, g_sz)
    T["sz_levels"] = np.unique(D)
    if D.max() < ROWS:
        lv, size = components(D, 1 if g_sz > 0 else 0)
        key, cnt = np.unique(lv.astype(np.int64) * (1 << 32) + size, return_counts=True)
        T["zones"] = np.stack([key >> 32, key & 0xFFFFFFFF, cnt], axis=1).astype(np.int64).reshape(-1, 3)
    return T


def move_count(T: dict, which, up: bool = True) -> dict:
    """A copy of T with ONE count moved to the neighbouring cell of its matrix: which = direction 0 .. 12 (a run one cell longer or
    shorter) or "zones" (a zone one cell larger or smaller).  The hook of the sensitivity test; None when the matrix has no count to move."""
    U = dict(T)
    if which == "zones":
        Z = T["zones"].copy()
        if len(Z) == 0:
            return None
        q = int(np.argmax(Z[:, 2]))
        lvl, size = int(Z[q, 0]), int(Z[q, 1])
        new = size + 1 if (up or size == 1) else size - 1
        Z[q, 2] -= 1
        Z = np.concatenate([Z[Z[:, 2] > 0], [[lvl, new, 1]]])
        key, inv = np.unique(Z[:, 0] * (1 << 32) + Z[:, 1], return_inverse=True)
        cnt = np.bincount(inv, weights=Z[:, 2]).astype(np.int64)
        U["zones"] = np.stack([key >> 32, key & 0xFFFFFFFF, cnt], axis=1).astype(np.int64)
        return U
    M = T["glrlm"][which].copy()
    if M.sum() == 0 or M.shape[1] < 2:
        return None
    i, j = np.unravel_index(int(np.argmax(M)), M.shape)
    j2 = j + 1 if (up and j + 1 < M.shape[1]) or j == 0 else j - 1
    M[i, j] -= 1
    M[i, j2] += 1
    U["glrlm"] = list(T["glrlm"])
    U["glrlm"][which] = M
    return U


def _levels(lv, g):
    return np.arange(1, int(lv.max()) + 1) if g == 0 else lv[lv > 0]


def glrlm_close(M: np.ndarray, I: np.ndarray, n_vox: int):
    """The 16 values of one direction from its run matrix (rows of I, columns up to the longest run)."""
    used = np.flatnonzero(M.sum(axis=0))
    Nr = int(used.max()) + 1 if len(used) else 0
    P = M[I][:, :Nr].astype(np.float64)
    tot = P.sum()
    if tot == 0:
        return [0.0] * N_CODES                             # every formula answers 0; RP = 0 / Np
    j = np.arange(1, Nr + 1, dtype=np.float64)[None, :]
    i = I.astype(np.float64)[:, None]
    i2, j2 = i * i, j * j
    si, sj = P.sum(axis=1), P.sum(axis=0)
    mu_g = (P / tot * i).sum()
    mu_r = (P / tot * j).sum()
    ent = fast_log10(P / tot + EPS) / LOG10_2
    return [(sj / j2[0]).sum() / tot, (P * j2).sum() / tot, (si * si).sum() / tot, (si * si).sum() / (tot * tot), (sj * sj).sum() / tot,
            (sj * sj).sum() / (tot * tot), tot / float(n_vox), (P / tot * ((i - mu_g) * (i - mu_g))).sum(), (P / tot * ((j - mu_r) * (j - mu_r))).sum(),
            -(P / tot * ent).sum(), (P / i2).sum() / tot, (P * i * i).sum() / tot, (P / (i2 * j2)).sum() / tot, (P * i2 / j2).sum() / tot,
            (P * j2 / i2).sum() / tot, (P * (i2 * j2)).sum() / tot]


def glszm_close(Z: np.ndarray, n_vox: int, soft_nan: float):
    """The 16 values from the zones (level, size, count): empty cells of the matrix add exactly 0 to every sum of this class."""
    if len(Z) == 0 or Z[:, 2].sum() == 0:
        return [soft_nan] * N_GLSZM                        # sum_p == 0 (3d_glszm.cpp:562-566)
    i, j, p = Z[:, 0].astype(np.float64), Z[:, 1].astype(np.float64), Z[:, 2].astype(np.float64)
    tot = p.sum()
    i2, j2 = i * i, j * j
    lv, inv = np.unique(Z[:, 0], return_inverse=True)
    si = np.bincount(inv, weights=p)
    sj = np.bincount(np.unique(Z[:, 1], return_inverse=True)[1], weights=p)
    li = lv.astype(np.float64)
    mu_z = (p / tot * j).sum()
    mu_g = (p / tot * i).sum()
    ent = fast_log10(p / tot + EPS) / LOG10_2
    return [(p / j2).sum() / tot, (p * j2).sum() / tot, (si * si).sum() / tot, (si * si).sum() / (tot * tot), (sj * sj).sum() / tot, (sj * sj).sum() / (tot * tot),
            tot / float(n_vox), (p / tot * ((i - mu_g) * (i - mu_g))).sum(), (p / tot * ((j - mu_z) * (j - mu_z))).sum(), -(p / tot * ent).sum(),
            (si / (li * li)).sum() / tot, (si * (li * li)).sum() / tot, (p / (i2 * j2)).sum() / tot, (p * i2 / j2).sum() / tot, (p * j2 / i2).sum() / tot,
            (p * i2 * j2).sum() / tot]


def columns(T: dict, s: _abi.Settings, t: _abi.VolZoneSettings) -> np.ndarray:
    """The 240 columns (GLRLM angled | GLRLM _AVE | GLSZM) from the matrices of one ROI."""
    nan = float(s.soft_nan)
    if T is None or T["flat"]:                             # no voxels; a flat ROI answers before it bins (3d_glrlm.cpp:115-136, 3d_glszm.cpp:476-480)
        ang = np.full((N_CODES, N_DIR), nan)
        return np.concatenate([ang.ravel(), [reduce13(row) for row in ang], np.full(N_GLSZM, nan)])
    g_rl, g_sz = grey_info(s, t)
    if "glrlm" in T:
        I = _levels(T["rl_levels"], g_rl)
        ang = np.array([glrlm_close(M, I, T["n"]) for M in T["glrlm"]]).T      # [code][direction]
    else:
        ang = np.full((N_CODES, N_DIR), np.nan)            # (more levels than the tables hold: the entry refuses the call)
    sz = glszm_close(T["zones"], T["n"], nan) if "zones" in T else [np.nan] * N_GLSZM
    return np.concatenate([ang.ravel(), [reduce13(row) for row in ang], sz])


def table(b: _abi.HostBatch3D, s: _abi.Settings, t: _abi.VolZoneSettings, zmask: int = _abi.VZONE_ALL) -> np.ndarray:
    full = np.array([columns(tables(b, r, s, t), s, t) for r in range(b.n_roi)]).reshape(b.n_roi, N_COL)
    sel = ([*range(N_GLRLM)] if zmask & _abi.VZONE_GLRLM else []) + ([*range(N_GLRLM, N_COL)] if zmask & _abi.VZONE_GLSZM else [])
    return full[:, sel]
