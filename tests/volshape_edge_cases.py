"""The clouds tests/test_volshape_gpu.py holds nyxhip_featurize_volumes_shape to tests/volshape_ref.py on: the smallest shapes at which
the kernels of roi_volshape.hip can go wrong.  Every builder returns an ROI dict for _abi.batch3d_from_rois.

  degenerate   clouds of rank < 3 (hull 0): one voxel, a pair, a line along z, a 5x4x1 plate, a body-diagonal needle, an oblique
               lattice plane inside a 6^3 box
  boxes        full boxes 2x2x2, 3x4x5, 9x9x9: every facet holds many coplanar and collinear candidates
  round        a lattice tetrahedron, lattice balls r = 3, 5, 8
  holes        a hollow shell, two disjoint blobs in one box, a box whose extreme corners carry intensity 0 (they count for the area and
               the volume and are left out of the hull)
  long         2 x 2 x 4000: 16-bit coordinates in the determinants, and 16000 candidates (the hull's workspace path)
  lds          a ball with a spike of single-voxel planes on its pole, sized so that the candidate count is LDS_CAND - 1 and
               LDS_CAND + 1 (kVshLdsCand of roi_volshape.h: the switch between the hull's storage in LDS and in the workspace)
"""
import numpy as np

from nyxus_amd import _abi
from tests import volshape_ref

LDS_CAND = 1024              # kVshLdsCand of roi_volshape.h


def from_mask(m, inten=None, rng=None):
    """an ROI from a mask [d, h, w]; intensities 1 .. 200 from rng (default: all 7), or `inten` per voxel"""
    z, y, x = np.nonzero(m)
    if inten is None:
        inten = rng.integers(1, 200, len(x)) if rng is not None else np.full(len(x), 7)
    return {"x": x, "y": y, "z": z, "inten": np.asarray(inten, np.uint32), "origin": (0, 0, 0), "box": m.shape[::-1]}


def full(w, h, d):
    return from_mask(np.ones((d, h, w), bool))


def ball_mask(r, extra=0):
    g = np.arange(-r, r + 1)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    m = x * x + y * y + z * z <= r * r
    if extra:                                              # a spike on the pole: `extra` planes of one voxel each
        m = np.concatenate([m, np.zeros((extra,) + m.shape[1:], bool)])
        m[2 * r + 1:, r, r] = True
    return m


def needle(n):
    i = np.arange(n)
    return {"x": i, "y": i, "z": i, "inten": np.full(n, 5, np.uint32), "origin": (0, 0, 0), "box": (n, n, n)}


def oblique_plane():
    """the lattice points of x + y + z == 7 inside a 6^3 box"""
    g = np.arange(6)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return from_mask(x + y + z == 7)


def tetrahedron():
    g = np.arange(6)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return from_mask(x + y + z <= 5)


def shell():
    m = ball_mask(6)
    inner = np.zeros_like(m)
    inner[2:11, 2:11, 2:11] = ball_mask(4)
    return from_mask(m & ~inner)


def two_blobs():
    m = np.zeros((9, 10, 12), bool)
    m[0:3, 0:4, 0:3] = True
    m[5:9, 6:10, 7:12] = ball_mask(2)[0:4, 0:4, :]
    return from_mask(m, rng=np.random.default_rng(17))


def dark_corners():
    """a full 5x4x6 box whose eight corners, and one whole edge, carry intensity 0"""
    m = np.ones((6, 4, 5), bool)
    v = np.full(m.shape, 9, np.uint32)
    for z in (0, 5):
        for y in (0, 3):
            for x in (0, 4):
                v[z, y, x] = 0
    v[0, 0, :] = 0
    return from_mask(m, inten=v[m])


def degenerate():
    one = {"x": [0], "y": [0], "z": [0], "inten": [3]}
    pair = {"x": [0, 1], "y": [0, 0], "z": [0, 0], "inten": [3, 4]}
    line = {"x": [0] * 7, "y": [0] * 7, "z": list(range(7)), "inten": list(range(1, 8))}
    return [one, pair, line, full(5, 4, 1), needle(6), oblique_plane()]


def lds_pair():
    """(the ROI one below the bound, the ROI one above): the largest ball under the bound with a spike that makes up the difference"""
    r = 8
    count = lambda m: len(volshape_ref.candidates(*[a for a in np.nonzero(m)[::-1]], np.ones(int(m.sum()))))
    while count(ball_mask(r + 1)) <= LDS_CAND - 1:
        r += 1
    c0 = count(ball_mask(r))
    out = []
    for want in (LDS_CAND - 1, LDS_CAND + 1):
        m = ball_mask(r, want - c0)
        assert count(m) == want
        out.append(from_mask(m))
    return out


_CACHE = {}


def groups():
    """name -> HostBatch3D"""
    if not _CACHE:
        rng = np.random.default_rng(23)
        _CACHE["degenerate"] = _abi.batch3d_from_rois(degenerate())
        _CACHE["boxes"] = _abi.batch3d_from_rois([full(2, 2, 2), full(3, 4, 5), full(9, 9, 9)])
        _CACHE["round"] = _abi.batch3d_from_rois([tetrahedron()] + [from_mask(ball_mask(r), rng=rng) for r in (3, 5, 8)])
        _CACHE["holes"] = _abi.batch3d_from_rois([shell(), two_blobs(), dark_corners()])
        _CACHE["long"] = _abi.batch3d_from_rois([full(2, 2, 4000)])
        _CACHE["lds"] = _abi.batch3d_from_rois(lds_pair())
    return _CACHE


_REF = {}


def reference(name):
    """(the restated table with soft_nan 0, 6 V as int64) of a group, computed once"""
    if name not in _REF:
        b = groups()[name]
        h6 = volshape_ref.hull6_of(b)
        T = np.array([volshape_ref.row(*volshape_ref.roi_arrays(b, r), hull6=int(h6[r])) for r in range(b.n_roi)])
        _REF[name] = (T, h6)
    return _REF[name]
