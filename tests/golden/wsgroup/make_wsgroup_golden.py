#!/usr/bin/env python3
"""Generates tests/golden/wsgroup/wsgroup_reference.npz and api_expected.json: the output of the reference's own ContourFeature,
Smoms2D_feature, Imoms2D_feature and RadialDistributionFeature in whole-slide mode (SINGLEROI) on the slides of tests/wsgroup_cases.py.
Only DATA is stored (211 doubles per slide, the centre and its squared radius, the reference's seconds); the slides are rebuilt from
seeds by tests/wsgroup_cases.py.

The reference classes are compiled OUTSIDE the repository: ref_wsgroup_driver.cpp (own code, next to this file) against the reference
sources where they lie, linked with the objects oracle/Makefile leaves in oracle/_ref/obj:

    REF=/root/reference/src/nyx; W=$(mktemp -d)
    g++ -std=c++20 -O2 -fPIC -w -I/opt/conda/include -c $REF/features/radial_distribution.cpp -o $W/radial_distribution.o
    g++ -std=c++20 -O2 -fPIC -shared -w -I$REF -Iinclude -I/opt/conda/include -o $W/libwsref.so \\
        tests/golden/wsgroup/ref_wsgroup_driver.cpp $W/radial_distribution.o $(find oracle/_ref/obj -name '*.o') \\
        /usr/lib/x86_64-linux-gnu/libtiff.so.5 -lpthread
    WSREF_SO=$W/libwsref.so python tests/golden/wsgroup/make_wsgroup_golden.py

The generator
  * asserts, on every pixel of every case, the identity the sweep kernel relies on: the least of the reference's four dist_to_segment
    equals min(x, w-1-x, y, h-1-y) exactly (integer operands, the root of a perfect square);
  * refuses to store a radial row where the reference is undefined (a 1 x 1 slide: max_sqdist == 0, a division by zero and a NaN
    converted to int) -- the stored row holds NaN there and `radial_defined` is False;
  * asserts that the reference's output is finite, or NaN / inf in recorded places (the all-zero slide's intensity moments).

api_expected.json: the column names of Nyxus(["*WHOLESLIDE*"]) as the reference's header code produces them
(output_2_buffer.cpp:316-445) for the twelve classes of the group (env_features.cpp:219-234), with the default four GLCM angles and four
Gabor filters, and which of them belong to the four blocks stored here.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
from nyxus_amd import _abi, _lib, featureset, featureset_morph  # noqa: E402
from tests import wsgroup_cases  # noqa: E402


def ref_row(lib, img):
    h, w = img.shape
    pix = np.ascontiguousarray(img.astype(np.uint32))
    out, info, sec = np.zeros(211), np.zeros(4), np.zeros(4)
    rc = lib.wsref_slide(pix.ctypes.data, w, h, out.ctypes.data, info.ctypes.data, sec.ctypes.data)
    assert rc == 0, rc
    return out, info, sec


def main():
    lib = C.CDLL(os.environ["WSREF_SO"])
    lib.wsref_slide.restype = C.c_int
    lib.wsref_slide.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    store = {}
    for name in wsgroup_cases.CASES:
        img = wsgroup_cases.image(name)
        row, info, sec = ref_row(lib, img)
        assert info[0] == 0, (name, "dist_to_segment differs from min(x, w-1-x, y, h-1-y) on", info[0], "pixels")
        defined = info[1] > 0
        assert defined == (img.size > 1), name
        if not defined:
            row[187:] = np.nan                                   # no radial row is stored where the reference is undefined
        finite = np.isfinite(row)
        assert (finite[187:].all() if defined else True) and finite[:7].all(), name
        if name not in wsgroup_cases.NAN_CASES:
            assert finite[:187].all(), (name, np.nonzero(~finite)[0])
        store[f"{name}__row"], store[f"{name}__centre"], store[f"{name}__seconds"] = row, info[1:], sec
        store[f"{name}__radial_defined"] = np.array(defined)
        print(f"{name}: {img.shape[1]} x {img.shape[0]} {img.dtype}, centre ({int(info[2])}, {int(info[3])}) r2 {int(info[1])}, non-finite {int((~finite).sum())}, "
              f"reference seconds {sec.sum():.4f}")
    np.savez_compressed(os.path.join(HERE, "wsgroup_reference.npz"), **store)
    # the reference's column names for the group: class by class in enum order, angles and filters expanded
    s = _abi.default_settings(64)
    angles = [s.glcm_angles[i] for i in range(s.glcm_n_angles)]
    cols = []
    group = (featureset.INTENSITY + featureset_morph.CONTOUR + featureset.GLCM_ANGLED + featureset.GLCM_AVE + featureset.GLRLM_ANGLED + featureset.GLRLM_AVE
             + featureset.GLSZM + featureset.GLDM + featureset.NGLDM + featureset.NGTDM + ["FRAC_AT_D", "GABOR", "MEAN_FRAC", "RADIAL_CV", "ZERNIKE2D"] + featureset.IMOMS)
    for c in group:
        if c in featureset.GLCM_ANGLED:
            cols += [f"{c}_{a}" for a in angles]
        elif c in featureset.GLRLM_ANGLED:
            cols += [f"{c}_{a}" for a in (0, 45, 90, 135)]
        elif c == "GABOR":
            cols += [f"GABOR_{i}" for i in range(s.gabor_n_filters)]
        elif c in featureset.RADIAL:
            cols += [f"{c}_{i}" for i in range(8)]
        elif c == "ZERNIKE2D":
            cols += [f"ZERNIKE2D_Z{i}" for i in range(30)]
        else:
            cols.append(c)
    json.dump({"features": ["*WHOLESLIDE*"], "codes": group, "columns": cols,
               "block_names": {"contour": featureset_morph.CONTOUR, "smoms": featureset.SMOMS, "imoms": featureset.IMOMS,
                               "radial": [f"{c}_{i}" for c in featureset.RADIAL for i in range(8)]}},
              open(os.path.join(HERE, "api_expected.json"), "w"))


if __name__ == "__main__":
    main()
