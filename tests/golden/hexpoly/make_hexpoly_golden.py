#!/usr/bin/env python3
"""Generates tests/golden/hexpoly/hexpoly_reference.npz and api_expected.json: the output of the reference's own
HexagonalityPolygonalityFeature (a) on the six inputs of every ROI of tests/hexpoly_cases.py and (b) on a seeded sweep of about 2000
synthetic six-tuples (hexpoly_cases.sweep).  Only DATA is stored: per row the seven numbers of hexpoly_ref.INPUTS (the pixel count, the
contour length and the five feature values the class reads) and its three outputs, raw.

The reference class is compiled OUTSIDE the repository: ref_hexpoly_driver.cpp (own code, next to this file) against the reference
sources where they lie, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    REF=/root/reference/src/nyx; W=$(mktemp -d)
    g++ -std=c++20 -O2 -fPIC -w -I/opt/conda/include -c $REF/features/hexagonality_polygonality.cpp -o $W/hexagonality_polygonality.o
    g++ -std=c++20 -O2 -fPIC -shared -w -I$REF -Iinclude -I/opt/conda/include -o $W/libhexpolyref.so \\
        tests/golden/hexpoly/ref_hexpoly_driver.cpp $W/*.o \\
        $(find oracle/_ref/obj -name '*.o') /usr/lib/x86_64-linux-gnu/libtiff.so.5 -lpthread
    HEXPOLYREF_SO=$W/libhexpolyref.so python tests/golden/hexpoly/make_hexpoly_golden.py

The inputs of (a) are those of tests/hexpoly_ref.inputs_of, i.e. of neighbors_ref, morph_ref and caliper_ref, each of which its own
fixtures pin to the reference's classes bit for bit.  Every output row is compared with tests/hexpoly_ref.closing before it is stored,
BIT FOR BIT (a NaN matching a NaN): the generator stops at the first difference.  It also asserts that the named branches occur: -1
rows for 0, 1 and 2 neighbors, for an empty contour and for a hull area of 0; rows beyond the tangent table; NaN and infinities in the
sweep; the hexagonality of the packed discs above that of the lattice's boxes.

The reference's Python package is not built here, so api_expected.json holds the driver-recorded hexagonality / polygonality columns
of one small stack with the reference's user-facing column names, the 108 codes of *ALL_MORPHOLOGY* in enum order and the stack's
labels; not-finite values are replaced by the soft NaN (0) as the reference's table writer replaces them.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
from tests import hexpoly_cases as hc, hexpoly_ref as hr  # noqa: E402


def load():
    lib = C.CDLL(os.environ["HEXPOLYREF_SO"])
    lib.hexpolyref_rows.restype = C.c_int
    lib.hexpolyref_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


def ref_rows(lib, X):
    X = np.ascontiguousarray(X, np.float64)
    out = np.zeros((len(X), 3))
    rc = lib.hexpolyref_rows(X.ctypes.data, len(X), out.ctypes.data)
    assert rc == 0, rc
    return out


def main():
    lib = load()
    store = {}
    sets = {name: hr.inputs_of(hc.batch(name), hc.radius(name)) for name in hc.CASES}
    sets["sweep"] = hc.sweep()
    for name, X in sets.items():
        T = ref_rows(lib, X)
        R = hr.closing_rows(X)
        bad = [r for r in range(len(X)) if not hr.same_bits(T[r], R[r])]
        assert not bad, (name, [(r, X[r].tolist(), T[r].tolist(), R[r].tolist()) for r in bad[:5]])
        store[f"{name}__in"], store[f"{name}__out"] = X, T
        gated = (T == -1).all(axis=1)
        print(f"{name}: {len(X)} rows, {int(gated.sum())} gated, {int(np.isnan(T).any(axis=1).sum())} with NaN, {int(np.isinf(T).any(axis=1).sum())} with inf, "
              f"neighbor counts {sorted(set(X[:, 2].astype(int).tolist()))[:12]}")
    lo = store["low_counts__in"][:, 2].astype(int).tolist()
    assert sorted(set(lo)) == [0, 1, 2] and (store["low_counts__out"] == -1).all()
    nc_in, nc_out = store["no_contour__in"], store["no_contour__out"]
    assert (nc_in[:, 1] == 0).sum() == 2 and (nc_out[nc_in[:, 1] == 0] == -1).all() and (nc_out[nc_in[:, 2] >= 3] != -1).all()
    assert sorted(set(store["lattice__in"][:, 2].astype(int).tolist())) == [3, 5, 8]
    assert store["beyond_table__in"][:, 2].max() > hr.TAN_TABLE_CAP
    S_in, S_out = store["sweep__in"], store["sweep__out"]
    for nb in (0, 1, 2, 3, 4, 5, 128, 129, 1000):
        assert (S_in[:, 2] == nb).any(), nb
    assert ((S_in[:, 4] == 0) & (S_out == -1).all(axis=1)).any() and ((S_in[:, 1] == 0) & (S_out == -1).all(axis=1)).any()
    live = S_in[:, 2] >= 3
    assert np.isnan(S_out[live]).any() and np.isinf(S_out[live]).any() and (S_in[live, 5] == 0).any() and (S_in[live, 3] == 0).any()
    hexd = hc.batch("hex_discs")
    mid = [int(np.nonzero(np.asarray(hexd.roi_label) == lab)[0][0]) for lab in hc.HEX_MIDDLE]
    assert (store["hex_discs__in"][mid, 2] == 6).all()
    assert store["hex_discs__out"][mid, 1].min() > store["lattice__out"][:, 1].max()
    np.savez_compressed(os.path.join(HERE, "hexpoly_reference.npz"), **store)
    b = hc.batch(hc.API_CASE)
    T = store[f"{hc.API_CASE}__out"]
    classes, codes = all_morphology_of_the_reference()
    api = {"case": hc.API_CASE, "neighbor_distance": hc.radius(hc.API_CASE), "labels": [int(v) for v in np.asarray(b.roi_label)],
           "all_morphology_classes": classes, "all_morphology": codes,
           "columns": list(hr.NAMES), "numeric": np.where(np.isfinite(T), T, 0.0).tolist()}
    assert len(codes) == 108 == len(set(codes)) and len(classes) == 16
    json.dump(api, open(os.path.join(HERE, "api_expected.json"), "w"))


def all_morphology_of_the_reference(ref=os.environ.get("NYXUS_REF", "/root/reference/src/nyx")):
    """(the classes FG2_MORPHOLOGY enables with their `featureset` members in the order of env_features.cpp, the union of the members in
    the order of the Feature2D enum), read from the reference's sources as text."""
    import glob
    import re
    env = open(os.path.join(ref, "env_features.cpp")).read()
    block = env[env.index("Fgroup2D::FG2_MORPHOLOGY)"):]
    block = block[:block.index("return true")]
    names = re.findall(r"enableFeatures\s*\((\w+)::featureset", block)
    headers = {h: open(h).read() for h in glob.glob(os.path.join(ref, "features", "*.h"))}
    classes = {}
    for cls in names:
        src = next(t for t in headers.values() if re.search(r"class\s+%s\b[^;]*\{" % cls, t))
        body = src[re.search(r"class\s+%s\b" % cls, src).start():]
        body = body[body.index("featureset"):]
        classes[cls] = re.findall(r"Feature2D::(\w+)", body[:body.index("};")])
    fs = open(os.path.join(ref, "featureset.h")).read()
    enum = fs[fs.index("enum class Feature2D"):]
    enum = re.sub(r"//[^\n]*", "", enum[enum.index("{") + 1:enum.index("};")])
    order = [t.split("=")[0].strip() for t in enum.split(",") if t.strip()]
    want = {c for members in classes.values() for c in members}
    return classes, [n for n in order if n in want]


if __name__ == "__main__":
    main()
