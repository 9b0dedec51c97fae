"""A numpy restatement of the reference's 3-D shape class (D3_SurfaceFeature::calculate, features/3d_surface.cpp:322-516) in the
reference's operation order, with the one ruling of DESIGN.md 4.5n: the hull columns hold the EXACT volume of the convex hull of the
centres of the voxels of non-zero intensity (0 where they span fewer than three dimensions), as an integer 6 V.

Two exact hulls, both in integers, neither the kernel's:
  hull6v_brute   every supporting plane of the cloud by enumeration of point triples; for small clouds (O(n^4)).
  hull6v         facet by facet: the two supporting planes through a hull edge are found by pivoting (vectorised over the points), the
                 points of a facet are ordered as a polygon by a 2-D monotone chain on an integer projection of the plane, and a facet
                 adds the cone it spans with a point strictly inside the hull (coordinates scaled by 4 so that point is a lattice point).
tests/test_volshape_cpu.py holds them against each other and against scipy.spatial.ConvexHull.

`candidates` restates which points the kernel hulls (roi_volshape.hip): per z-plane the hull vertices of the (y, x) row extremes;
`contour_points` which points the reference hulls (its build_contour_imp, restated).
Eigen columns: the covariance in the reference's order (helpers.cpp:9-66), the eigenvalues by numpy.linalg.eigvalsh; the rank of the
cloud is decided from the inputs alone (`rank`, exact integers) and an eigenvalue beyond it is 0, as is every eigen column of one voxel
(the reference's solver does not converge on the NaN matrix there and the class writes 0)."""
from itertools import combinations

import numpy as np

from nyxus_amd import _abi

NAMES = ["3AREA", "3AREA_2_VOLUME", "3COMPACTNESS1", "3COMPACTNESS2", "3MESH_VOLUME", "3SPHERICAL_DISPROPORTION", "3SPHERICITY", "3VOLUME_CONVEXHULL",
         "3VOXEL_VOLUME", "3MAJOR_AXIS_LEN", "3MINOR_AXIS_LEN", "3LEAST_AXIS_LEN", "3ELONGATION", "3FLATNESS"]
COL = {n: i for i, n in enumerate(NAMES)}
HULL = [COL["3MESH_VOLUME"], COL["3VOLUME_CONVEXHULL"]]
CLOSED = [COL[n] for n in ("3AREA_2_VOLUME", "3COMPACTNESS1", "3COMPACTNESS2", "3SPHERICAL_DISPROPORTION", "3SPHERICITY", "3VOXEL_VOLUME")]
LENS = [COL[n] for n in ("3MAJOR_AXIS_LEN", "3MINOR_AXIS_LEN", "3LEAST_AXIS_LEN")]
RATIOS = [COL["3ELONGATION"], COL["3FLATNESS"]]


# ---- exact integer geometry ---------------------------------------------------------------------------------------------------------
def _det3(a, b, c):
    """det of rows a, b, c; a, b, c: int64 arrays [..., 3] (broadcast)"""
    return (a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]) - a[..., 1] * (b[..., 0] * c[..., 2] - b[..., 2] * c[..., 0]) +
            a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]))


def orient(a, b, c, D):
    """det(b - a, c - a, d - a) for every row d of D"""
    return _det3(b - a, c - a, D - a)


def rank(P) -> int:
    """The exact rank of the centred coordinates of the integer points P [n, 3]: 0 a point, 1 a line, 2 a plane, 3 a solid."""
    P = np.asarray(P, np.int64).reshape(-1, 3)
    if len(P) == 0:
        return 0
    D = P - P[0]
    nz = np.flatnonzero(D.any(axis=1))
    if len(nz) == 0:
        return 0
    u = D[nz[0]]
    cr = np.cross(u, D)
    off = np.flatnonzero(cr.any(axis=1))
    if len(off) == 0:
        return 1
    n = cr[off[0]]
    return 3 if (D @ n).any() else 2


def _polygon(P, idx, normal):
    """The points P[idx] of one plane as a convex polygon: the indices of its vertices in order (collinear points dropped), by a monotone
    chain on the projection that drops the coordinate of the normal's largest component."""
    k = int(np.argmax(np.abs(normal)))
    ax = [a for a in range(3) if a != k]
    pts = sorted((int(P[i, ax[0]]), int(P[i, ax[1]]), int(i)) for i in idx)
    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h
    lo, up = half(pts), half(pts[::-1])
    return [p[2] for p in lo[:-1] + up[:-1]]


def _cone(P4, poly, o) -> int:
    """|the fan sum| of the polygon against the apex o: 6 x the volume of the cone, in the scale of P4"""
    a = P4[poly[0]] - o
    s = 0
    for u, v in zip(poly[1:-1], poly[2:]):
        s += int(_det3(a, P4[u] - o, P4[v] - o))
    return abs(s)


def _inner(P):
    """(4 P, a lattice point of that scale strictly inside the hull): the sum of four points that span a solid"""
    D = P - P[0]
    i1 = int(np.flatnonzero(D.any(axis=1))[0])
    cr = np.cross(D[i1], D)
    i2 = int(np.flatnonzero(cr.any(axis=1))[0])
    i3 = int(np.flatnonzero(D @ cr[i2])[0])
    return 4 * P, P[0] + P[i1] + P[i2] + P[i3]


def _pivot(P, u, v, sign):
    """The points of the supporting plane through the edge (u, v) that has every point on the side `sign` (or on it): (indices, normal)."""
    a, b = P[u], P[v]
    cr = np.cross(b - a, P - a)
    c = int(np.flatnonzero(cr.any(axis=1))[0])
    for _ in range(len(P) + 1):
        t = orient(a, b, P[c], P) * sign
        if (t >= 0).all():
            return np.flatnonzero(t == 0), cr[c]
        c = int(np.argmin(t))
    raise AssertionError("pivot did not settle")


def hull6v(P) -> int:
    """6 x the volume of the convex hull of the integer points P [n, 3], exact; 0 for a cloud of rank < 3."""
    P = np.unique(np.asarray(P, np.int64).reshape(-1, 3), axis=0)
    if rank(P) < 3:
        return 0
    P4, o = _inner(P)
    # a first hull edge: the supporting plane through the smallest point a (np.unique sorts by x, y, z) and the direction ez
    a = P[0]
    D = P - a
    xy = np.flatnonzero(D[:, :2].any(axis=1))
    c = int(xy[0])
    for _ in range(len(P) + 1):
        t = D[c, 0] * D[:, 1] - D[c, 1] * D[:, 0]          # det(ez, c - a, d - a)
        if (t >= 0).all():
            break
        c = int(np.argmin(t))
    face = np.flatnonzero(t == 0)
    poly = _polygon(P, face, np.array([D[c, 1], -D[c, 0], 0]))
    at = poly.index(0)
    edges, seen, total = [(0, poly[(at + 1) % len(poly)])], set(), 0
    done = set()
    while edges:
        u, v = edges.pop()
        if (min(u, v), max(u, v)) in done:
            continue
        done.add((min(u, v), max(u, v)))
        for sign in (1, -1):
            idx, normal = _pivot(P, u, v, sign)
            key = tuple(idx)
            if key in seen:
                continue
            seen.add(key)
            poly = _polygon(P, idx, normal)
            total += _cone(P4, poly, o)
            edges += [(poly[i], poly[(i + 1) % len(poly)]) for i in range(len(poly))]
    assert total % 64 == 0
    return total // 64


def hull6v_brute(P) -> int:
    """6 x the volume of the convex hull by enumeration: every plane through three points that has all points on one side is a facet's."""
    P = np.unique(np.asarray(P, np.int64).reshape(-1, 3), axis=0)
    if rank(P) < 3:
        return 0
    P4, o = _inner(P)
    seen, total = set(), 0
    for i, j, k in combinations(range(len(P)), 3):
        t = orient(P[i], P[j], P[k], P)
        if not t.any() or ((t > 0).any() and (t < 0).any()):
            continue
        idx = np.flatnonzero(t == 0)
        if tuple(idx) in seen:
            continue
        seen.add(tuple(idx))
        total += _cone(P4, _polygon(P, idx, np.cross(P[j] - P[i], P[k] - P[i])), o)
    assert total % 64 == 0
    return total // 64


def candidates(x, y, z, inten) -> np.ndarray:
    """The points the kernel hulls [n, 3] (x, y, z): per z-plane the vertices of the 2-D hull of the plane's voxels of non-zero
    intensity, from the smallest and the largest x of every (z, y) row."""
    lit = np.asarray(inten) != 0
    x, y, z = (np.asarray(a, np.int64)[lit] for a in (x, y, z))
    out = []
    for zz in np.unique(z):
        m = z == zz
        rows = {}
        for xx, yy in zip(x[m], y[m]):
            lo, hi = rows.get(int(yy), (int(xx), int(xx)))
            rows[int(yy)] = (min(lo, int(xx)), max(hi, int(xx)))
        pts = sorted({(lo, yy) for yy, (lo, hi) in rows.items()} | {(hi, yy) for yy, (lo, hi) in rows.items()})
        P2 = np.array([(px, py, 0) for px, py in pts], np.int64)
        poly = _polygon(P2, range(len(pts)), np.array([0, 0, 1])) if len(pts) > 1 else [0]
        out += [(pts[i][0], pts[i][1], int(zz)) for i in poly]
    return np.array(sorted(set(out)), np.int64).reshape(-1, 3)


def contour_points(x, y, z, inten) -> np.ndarray:
    """The points the REFERENCE hulls [n, 3]: per z-plane the border its build_contour_imp traces (3d_surface.cpp:11-202), restated, in
    its order.  The plane's voxels -- all of them, intensity 0 included -- go into an image padded by one cell; a raster scan keeps an
    `inside` flag (set on meeting a traced border, cleared on the next blank cell) and, at a voxel met while outside, follows the
    border through the 8-neighbourhood clockwise from that voxel until it returns to it (Moore tracing with Jacob's stopping
    criterion: the start re-entered from the west, or met a third time) or finds no neighbour at all.  Border voxels of intensity 0 are
    dropped at the end."""
    x, y, z, inten = (np.asarray(a, np.int64) for a in (x, y, z, inten))
    x0, y0 = int(x.min()), int(y.min())
    W, H = int(x.max()) - x0 + 1, int(y.max()) - y0 + 1
    P = W + 2
    step = [(-1, 7), (-3 - W, 7), (-W - 2, 1), (-1 - W, 1), (1, 3), (3 + W, 3), (W + 2, 5), (1 + W, 5)]   # (offset, where to look next)
    out = []
    for zz in np.unique(z):
        idx = np.flatnonzero(z == zz)
        img = np.zeros((H + 2) * P, np.int64)
        img[(x[idx] - x0 + 1) + (y[idx] - y0 + 1) * P] = idx + 1
        border = np.zeros_like(img)
        inside = False
        for pos in range(len(img)):
            if border[pos] and not inside:
                inside = True
            elif img[pos] and inside:
                continue
            elif not img[pos] and inside:
                inside = False
            elif img[pos] and not inside:
                border[pos] = img[pos]
                at, look, start, met, turns = pos, 1, pos, 0, 0
                while True:
                    nxt, after = at + step[look - 1][0], step[look - 1][1]
                    if img[nxt]:
                        if nxt == start:
                            met += 1
                            if after == 1 or met >= 3:
                                inside = True
                                break
                        look, at, turns = after, nxt, 0
                        border[nxt] = img[nxt]
                    else:
                        look = 1 + look % 8
                        if turns > 8:
                            break
                        turns += 1
        keep = border[border != 0] - 1
        out += [int(i) for i in keep if inten[i] != 0]
    return np.stack([x[out], y[out], z[out]], axis=1) if out else np.zeros((0, 3), np.int64)


# ---- the class ----------------------------------------------------------------------------------------------------------------------
def _seq_sum(v) -> float:
    """a sum in the order std::accumulate adds (numpy's cumsum is sequential; its sum is pairwise)"""
    v = np.asarray(v, np.float64)
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


def exposed_faces(x, y, z) -> int:
    vox = set(zip(map(int, x), map(int, y), map(int, z)))
    return sum((vx + dx, vy + dy, vz + dz) not in vox for vx, vy, vz in zip(map(int, x), map(int, y), map(int, z))
               for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)))


def covariance(x, y, z) -> np.ndarray:
    """Pixel3::calc_cov_matrix (pixel.cpp:247-259) over calc_cov_matrix (helpers.cpp:9-66): centre on the centroid, then the sample
    covariance about the means of the centred columns"""
    n = len(x)
    T = np.stack([np.asarray(c, np.float64) - _seq_sum(c) / n for c in (x, y, z)], axis=1)
    mean = [_seq_sum(T[:, j]) / n for j in range(3)]
    K = np.zeros((3, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(3):
            for j in range(i, 3):
                K[i, j] = K[j, i] = np.float64(_seq_sum((T[:, i] - mean[i]) * (T[:, j] - mean[j]))) / np.float64(n - 1)
    return K


def eigenvalues(x, y, z) -> np.ndarray:
    """descending, clamped at 0, those beyond the exact rank of the cloud 0; one voxel: all 0"""
    if len(x) < 2:
        return np.zeros(3)
    L = np.maximum(np.linalg.eigvalsh(covariance(x, y, z))[::-1], 0.0)
    L[rank(np.stack([x, y, z], axis=1)):] = 0.0
    return L


def row(x, y, z, inten, soft_nan: float = 0.0, hull6=None) -> np.ndarray:
    """The 14 columns of one ROI (box-relative or absolute coordinates alike).  hull6: a 6 V computed elsewhere."""
    n = len(x)
    if n == 0:
        return np.full(14, soft_nan)
    o = np.zeros(14)
    vol = _seq_sum(np.full(n, 4. / 3. * np.pi * (1. / 8.))) / 0.5236
    area = float(exposed_faces(x, y, z))
    if hull6 is None:
        hull6 = hull6v(candidates(x, y, z, inten))
    o[COL["3AREA"]] = area
    o[COL["3VOXEL_VOLUME"]] = vol
    o[HULL] = hull6 / 6.0
    o[COL["3AREA_2_VOLUME"]] = area / vol
    o[COL["3COMPACTNESS1"]] = vol / np.sqrt(np.pi * area * area * area)
    o[COL["3COMPACTNESS2"]] = 36. * np.pi * vol * vol / (area * area * area)
    o[COL["3SPHERICAL_DISPROPORTION"]] = area / np.power(36. * np.pi * vol * vol, 1. / 3.)
    o[COL["3SPHERICITY"]] = np.power(36. * np.pi * vol * vol, 1. / 3.) / area
    L = eigenvalues(np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(z, np.int64))
    o[LENS] = 4.0 * np.sqrt(L)
    o[RATIOS] = np.sqrt(L[1:] / L[0]) if L[0] > 0 else 0.0
    return o


def roi_arrays(b: _abi.HostBatch3D, r: int):
    a, e = int(b.px_offset[r]), int(b.px_offset[r + 1])
    return b.x[a:e].astype(np.int64), b.y[a:e].astype(np.int64), b.z[a:e].astype(np.int64), b.inten[a:e]


def hull6_of(b: _abi.HostBatch3D) -> np.ndarray:
    """6 V of every ROI as int64"""
    return np.array([hull6v(candidates(*roi_arrays(b, r))) for r in range(b.n_roi)], np.int64)


def table(b: _abi.HostBatch3D, s: _abi.Settings) -> np.ndarray:
    return np.array([row(*roi_arrays(b, r), soft_nan=s.soft_nan) for r in range(b.n_roi)]).reshape(b.n_roi, 14)
