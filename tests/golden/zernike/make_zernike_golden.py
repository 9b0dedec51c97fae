"""Writes tests/golden/zernike/zernike_exact.json: for every case of tests/zernike_cases.py the 30 exact ZERNIKE2D magnitudes
(tests/zernike_ref.exact: mpmath, 50 digits) as hex floats, a hash of the case's inputs, its pixel count and its kept-pixel count.
Run once, from the repository root, when a case is added or changed (a few minutes; needs mpmath):

    python tests/golden/zernike/make_zernike_golden.py
"""
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import zernike_cases as zc  # noqa: E402
from tests import zernike_ref as zr  # noqa: E402


def one(name):
    roi = zc.roi(name)
    w, h = zc.box(roi)
    mem = zc.members(roi)
    return name, {"hash": zr.input_hash(roi, w, h), "box": [w, h], "npx": len(roi["x"]), "kept": mem["n_kept"],
                  "exact": [float(v).hex() for v in zr.exact(mem)]}


def main():
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        cases = dict(pool.map(one, list(zc.CASES), chunksize=1))
    out = {"digits": 50, "order": zr.ORDER, "pairs": zr.PAIRS, "cases": {k: cases[k] for k in zc.CASES}}
    with open(zc.GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)
        f.write("\n")
    print(f"{len(cases)} cases -> {zc.GOLDEN}")


if __name__ == "__main__":
    main()
