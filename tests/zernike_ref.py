"""TEST INFRASTRUCTURE -- ZERNIKE2D stated exactly, for tests/test_zernike_cpu.py and tests/test_zernike_gpu.py.

The HIP kernel (roi_zernike_kernel, nyxus_amd/csrc/roi_shape.hip) does not run the reference's per-pixel radial recurrence: it adds up 30
complex power sums and recombines them once per ROI.  Two different algorithms are held to the operation itself, not to each other:

members()   the one discontinuous step -- which pixels lie in the unit disc -- in IEEE double, operation by operation as the reference
            performs it (features/zernike.cpp:216-230, :262-274).  Every case keeps sum v and sum (i + 1) v below 2^53, so the reference's
            double accumulation and the kernel's 64-bit integer sums are the same numbers whatever the order.
exact()     the 30 magnitudes |A_nm| of the kept pixels at 50 digits (mpmath), the doubles x, y and f = v / sum v taken as exact inputs.
unit()      2^-52 (n + 1) / pi S_nm, S_nm = sum_s |coefficient of r^(n - 2 s) in R_nm|: one rounding of the largest magnitude a term of
            either algorithm can reach (|sum f g| <= sum f <= 1 for |g| <= 1 on r <= 1).
bound()     L(npx) = 32 + ceil(npx / 256) units -- derived, not measured: ~15 roundings in a pixel's product chain, a thread's serial sum of
            ceil(npx / 256) terms, 8 tree levels, the recombination.  Absolute, so a column whose true value is 1e-9 is still checked.
"""
from __future__ import annotations

import hashlib
import math
from fractions import Fraction

import numpy as np

ORDER = 9
PAIRS = [(n, m) for n in range(ORDER + 1) for m in range(n + 1) if (n - m) % 2 == 0]     # the reference's output order (:330-341)
assert len(PAIRS) == 30
DBL_EPSILON = 2.0 ** -52


def coefficients(n, m):
    """R_nm(r) = sum_s c_s r^(n - 2 s): [(n - 2 s, c_s)], exact integers."""
    f = math.factorial
    return [(n - 2 * s, (-1) ** s * f(n - s) // (f(s) * f((n + m) // 2 - s) * f((n - m) // 2 - s))) for s in range((n - m) // 2 + 1)]


def S(n, m):
    return sum(abs(c) for _, c in coefficients(n, m))


assert S(9, 1) == 681 and S(8, 0) == 321


def unit(n, m):
    return 2.0 ** -52 * (n + 1) / math.pi * S(n, m)


UNITS = np.array([unit(n, m) for n, m in PAIRS])


def bound(npx):
    """L(npx), in units."""
    return 32 + -(-int(npx) // 256)


def members(x, y, v, w, h):
    """The reference's membership decision in IEEE double.  x, y: box-relative integer coordinates, v: intensities, w, h: the box.
    Returns a dict: keep (mask over the cloud), X, Y, r2, r (doubles of every cloud pixel), sum, m10, m01 (Python ints), n_kept."""
    x = np.asarray(x, np.int64)
    y = np.asarray(y, np.int64)
    v = np.asarray(v, np.int64)
    m00 = int(v.sum())
    m10 = int(((x + 1) * v).sum())
    m01 = int(((y + 1) * v).sum())
    assert 0 < m00 < 2 ** 53 and m10 < 2 ** 53 and m01 < 2 ** 53, "the sums must be exact in double"
    cx = float(m10) / float(m00)                                             # moment10 / moment00 (:227-228)
    cy = float(m01) / float(m00)
    rad = float(min(int(w), int(h)))                                         # N = min(width, height), rad = N (:185, :194)
    X = ((x + 1).astype(np.float64) - cx) / rad                              # :262
    Y = ((y + 1).astype(np.float64) - cy) / rad                              # :270
    xx = X * X                                                               # two products, one sum: each rounded (no fused multiply-add)
    yy = Y * Y
    r2 = xx + yy                                                             # :271
    r = np.sqrt(r2)                                                          # :272
    keep = ~((r < DBL_EPSILON) | (r > 1.0))                                  # :273
    return {"keep": keep, "X": X, "Y": Y, "r2": r2, "r": r, "sum": m00, "m10": m10, "m01": m01, "v": v, "n_kept": int(keep.sum())}


def _round(fr):
    """A Fraction rounded to the nearest double (ties to even: int / int division in Python is correctly rounded)."""
    return fr.numerator / fr.denominator


def r2_fused(X, Y):
    """x * x + y * y with one product fused into the sum, both ways round: (fma(x, x, y * y), fma(y, y, x * x)), exactly."""
    X, Y = float(X), float(Y)
    a = _round(Fraction(X) * Fraction(X) + Fraction(Y * Y))
    b = _round(Fraction(Y) * Fraction(Y) + Fraction(X * X))
    return a, b


def decision(r2):
    """True: kept."""
    r = math.sqrt(r2)
    return not (r < DBL_EPSILON or r > 1.0)


def exact(mem, dps=50):
    """|A_nm| of the kept pixels for the 30 pairs, as doubles rounded from the 50-digit values.
    A_nm = (n + 1) / pi sum f R_nm(r) e^{-i (m + 1) theta}; the reference's COST[m] / SINT[m] are cos / sin of (m + 1) theta (:280-286).
    By linearity the sum over pixels is taken per power of r first: sum f r^k e^{-i (m + 1) theta}, then the closed form's integer
    coefficients -- at 50 digits the order of a finite sum is immaterial."""
    import mpmath
    from mpmath import mpf
    with mpmath.workdps(dps):
        keep = mem["keep"]
        total = float(mem["sum"])
        zero = mpf(0)
        sr = {(k, m): zero for n, m in PAIRS for k, _ in coefficients(n, m)}
        si = dict(sr)
        keys = sorted(sr)
        for X, Y, v in zip(mem["X"][keep].tolist(), mem["Y"][keep].tolist(), mem["v"][keep].tolist()):
            if v == 0:
                continue
            f = mpf(float(v) / total)                                        # :291, a double
            x, y = mpf(X), mpf(Y)
            r = mpmath.sqrt(x * x + y * y)
            ur, ui = x / r, -y / r                                           # e^{-i theta}
            rp = [mpf(1)]
            for _ in range(ORDER):
                rp.append(rp[-1] * r)
            er, ei = [ur], [ui]                                              # e^{-i (m + 1) theta}, m = 0 .. 9
            for _ in range(ORDER):
                er.append(er[-1] * ur - ei[-1] * ui)
                ei.append(ei[-1] * ur + er[-2] * ui)
            for k, m in keys:
                w = f * rp[k]
                sr[k, m] += w * er[m]
                si[k, m] += w * ei[m]
        out = []
        for n, m in PAIRS:
            ar = sum((c * sr[k, m] for k, c in coefficients(n, m)), zero)
            ai = sum((c * si[k, m] for k, c in coefficients(n, m)), zero)
            out.append(float((n + 1) / mpmath.pi * mpmath.sqrt(ar * ar + ai * ai)))
        return np.array(out)


def input_hash(roi, w, h):
    """A case's inputs: box-relative coordinates, intensities and the box."""
    hsh = hashlib.sha256()
    hsh.update(np.asarray([w, h], np.uint32).tobytes())
    for key, dt in (("x", np.uint16), ("y", np.uint16), ("inten", np.uint32)):
        hsh.update(np.ascontiguousarray(roi[key], dt).tobytes())
    return hsh.hexdigest()[:32]
