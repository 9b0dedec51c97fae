"""The recorded cases of the volume shape entry (tests/golden/volshape, tests/test_volshape_cpu.py, tests/test_volshape_gpu.py): the batches
handed to the reference's own class, the tolerances, and how two tables are compared.

Every recorded ROI is one on which the reference's float quickhull finds the exact hull (make_volshape_golden.py asserts it; DESIGN.md
4.5n): full boxes, a lattice ball of r = 3, a lattice tetrahedron, the rank-deficient clouds it survives (one voxel, a pair, a line along an axis: it reports
a degenerate shell and leaves 0; on a plane or an oblique line a build with assertions aborts in quickhull.hpp's create_initial_simplex,
so those are held to the restatement alone) and small random clouds.  INEXACT names the clouds on which it does not: they are recorded side by side with the exact value
under "<case>__reference_inexact" and never compared.

TOL          3VOXEL_VOLUME and the closed forms, relative; the eigen columns as squares: (len / 4)^2 within TOL x lambda_max and the squared
             ratios within TOL absolute (a square root blows an error up without bound near a zero eigenvalue).  1e-10 against the kernel
             (tests/test_volshape_gpu.py states why); the restatement follows the reference's operation order and is held to
             TOL_RESTATED = 1e-12 on the closed forms.
HULL_AGREE   the relative difference under which the reference's hull volume counts as equal to the exact one.  The reference sums
             det4 / 6 in fp64 over float vertices against an fp64 centroid: where its hull is right the difference is rounding (the
             recording script measures at most a few 1e-15), where it is wrong it is a missing or spurious facet (the smallest it
             measures is above 1e-4).  1e-9 lies orders of magnitude from both.
"""
import numpy as np

from nyxus_amd import _abi
from tests import volshape_edge_cases as E
from tests import volshape_ref as R

TOL = 1e-10
TOL_RESTATED = 1e-12
HULL_AGREE = 1e-9
N_COL = 14
CASES = ["boxes", "round", "flat", "clouds"]
INEXACT = ["ball5", "ball8", "ellipsoid"]


def settings(soft_nan: float = 0.0) -> _abi.Settings:
    s = _abi.default_settings(64)
    s.soft_nan = soft_nan
    return s


def _clouds():
    """random clouds in boxes of sides 2 .. 5 at density 0.5, intensities 0 .. 4 (a fifth of the voxels carries 0)"""
    rng = np.random.default_rng(1405)
    rois = []
    while len(rois) < 12:
        d, h, w = rng.integers(2, 6, 3)
        m = rng.random((d, h, w)) < 0.5
        if m.sum() < 2:
            continue
        rois.append(E.from_mask(m, inten=rng.integers(0, 5, int(m.sum()))))
    return rois


def ellipsoid_mask(a=5, b=7, c=9):
    """the 10 x 14 x 18 ellipsoid of DESIGN.md 4.5n: voxel centres at half-integers inside x^2 / a^2 + y^2 / b^2 + z^2 / c^2 <= 1"""
    z, y, x = np.meshgrid(np.arange(-c, c) + 0.5, np.arange(-b, b) + 0.5, np.arange(-a, a) + 0.5, indexing="ij")
    return (x / a) ** 2 + (y / b) ** 2 + (z / c) ** 2 <= 1.0


_CACHE = {}


def batch(name: str) -> _abi.HostBatch3D:
    if name not in _CACHE:
        rng = np.random.default_rng(77)
        build = {
            "boxes": lambda: [E.full(2, 2, 2), E.full(3, 4, 5), E.full(6, 6, 6), E.full(7, 2, 3)],
            "round": lambda: [E.from_mask(E.ball_mask(3), rng=rng), E.tetrahedron()],
            "flat": lambda: E.degenerate()[:3],
            "clouds": _clouds,
            "ball5": lambda: [E.from_mask(E.ball_mask(5))],
            "ball8": lambda: [E.from_mask(E.ball_mask(8))],
            "ellipsoid": lambda: [E.from_mask(ellipsoid_mask())],
        }[name]
        _CACHE[name] = _abi.batch3d_from_rois(build())
    return _CACHE[name]


def ranks(b: _abi.HostBatch3D) -> np.ndarray:
    """the exact rank of every ROI's cloud, from the inputs alone (all voxels: the covariance reads them all)"""
    return np.array([R.rank(np.stack(R.roi_arrays(b, r)[:3], axis=1)) for r in range(b.n_roi)])


def eigen_compared(b: _abi.HostBatch3D) -> np.ndarray:
    """[n_roi x 14] True where an eigen column is compared with the reference: a rank-deficient cloud leaves the solver's rounding in the
    eigenvalues beyond its rank (and the NaN matrix of one voxel all of them), so those are pinned to the restatement's 0 instead"""
    ok = np.ones((b.n_roi, N_COL), bool)
    for r, k in enumerate(ranks(b)):
        ok[r, R.LENS[k:]] = False
        ok[r, R.RATIOS[max(k - 1, 0):]] = False
    return ok


def figures(got: np.ndarray, want: np.ndarray, mask=None) -> dict:
    """The largest differences by the rules above: 'closed' relative, 'lens' as squares relative to lambda_max, 'ratios' as squares,
    'hull' relative (0 against 0 counts as 0).  mask [n x 14]: the entries that are compared."""
    got, want = np.asarray(got, np.float64).reshape(-1, N_COL), np.asarray(want, np.float64).reshape(-1, N_COL)
    mask = np.ones(got.shape, bool) if mask is None else mask
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - want) / np.abs(want)
        rel[got == want] = 0.0
        lam = (want[:, R.LENS] / 4.0) ** 2
        top = np.maximum(lam.max(axis=1, keepdims=True), np.finfo(float).tiny)
        lens = np.abs((got[:, R.LENS] / 4.0) ** 2 - lam) / top
        ratios = np.abs(got[:, R.RATIOS] ** 2 - want[:, R.RATIOS] ** 2)
    pick = lambda v, cols: float(np.nan_to_num(np.where(mask[:, cols], v, 0.0), nan=np.inf).max(initial=0.0))
    return {"closed": pick(rel[:, R.CLOSED], R.CLOSED), "hull": pick(rel[:, R.HULL], R.HULL), "lens": pick(lens, R.LENS), "ratios": pick(ratios, R.RATIOS)}
