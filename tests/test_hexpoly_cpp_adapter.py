"""HexagonalityPolygonalityFeature of the C++ plugin adapter (include/nyxhip_feature_method.hpp): compiles on the CPU; on the GPU the
reference-style unit test (tests/cpp/test_hexpoly_method.cpp) reproduces, bit for bit, the values recorded from the reference's class
for the ROIs of one image of tests/hexpoly_cases.py through HexagonalityPolygonalityFeature::manual_reduce."""
import os
import subprocess

import numpy as np
import pytest

from tests import hexpoly_cases as hc, hexpoly_ref as hr, neighbors_cases as nc, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_hexpoly_method.bin")


def _build():
    lib = os.path.join(ROOT, "nyxus_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "test_hexpoly_method.cpp"),
           "-o", BIN, "-L", lib, "-lnyxhip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_hexpoly_adapter_compiles_and_links_against_the_abi():
    _build()
    r = subprocess.run([BIN, "--compile-check"], capture_output=True, text=True)
    assert r.returncode == 0 and "compiled" in r.stdout


@pytest.mark.gpu
def test_reference_style_hexpoly_test_passes_on_gpu(tmp_path):
    if not os.path.exists(BIN):
        _build()
    name = "no_contour"                                  # four neighbors, two neighbors (-1), two ROIs without a contour (-1)
    lab = hc.images(name)[0]
    rois = synth.rois_from_tile(nc.intensity(lab, 500), lab)
    want = hc.golden()[name][1]
    gated = (want == -1).all(axis=1)
    assert len(rois) == len(want) == 10 and gated.sum() == 6 and np.isfinite(want).all()
    assert hr.same_bits(want, hr.table(hc.batch(name), hc.radius(name)))
    rois, want = rois[::-1], want[::-1]                  # handed over in descending order: manual_reduce sorts the labels itself
    text = "%d %d\n" % (hc.radius(name), len(rois))
    for r in rois:
        text += "%d %d\n" % (r["label"], len(r["x"])) + "".join("%d %d %d\n" % t for t in zip(r["x"], r["y"], r["inten"]))
    text += "\n".join(" ".join(repr(float(v)) for v in row) for row in want) + "\n"
    path = tmp_path / "case.txt"
    path.write_text(text)
    r = subprocess.run([BIN, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
