"""NeighborsFeature of the C++ plugin adapter (include/nyxhip_feature_method.hpp): compiles on the CPU; on the GPU the reference-style
unit test (tests/cpp/test_neighbors_method.cpp) reproduces the values recorded from the reference's class for the ROIs of one image of
tests/neighbors_cases.py through NeighborsFeature::manual_reduce."""
import os
import subprocess

import numpy as np
import pytest

from tests import neighbors_cases as nc, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_neighbors_method.bin")


def _build():
    lib = os.path.join(ROOT, "nyxus_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "test_neighbors_method.cpp"),
           "-o", BIN, "-L", lib, "-lnyxhip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_neighbors_adapter_compiles_and_links_against_the_abi():
    _build()
    r = subprocess.run([BIN, "--compile-check"], capture_output=True, text=True)
    assert r.returncode == 0 and "compiled" in r.stdout


@pytest.mark.gpu
def test_reference_style_neighbors_test_passes_on_gpu(tmp_path):
    if not os.path.exists(BIN):
        _build()
    name, radius = "ties", 5                             # three neighbors at equal distances, a blob inside a ring: ties, angles, a deviation
    lab = nc.images(name)[0]
    rois = synth.rois_from_tile(nc.intensity(lab, 500), lab)
    want = nc.golden()[(name, radius)][:, :9]
    assert len(rois) == len(want) == 6 and want[:, 0].max() == 3 and (want[:, 7] > 0).any()
    rois = rois[::-1]                                    # handed over in descending order: manual_reduce sorts the labels itself
    text = "%d %d\n" % (radius, len(rois))
    for r in rois:
        text += "%d %d\n" % (r["label"], len(r["x"])) + "".join("%d %d %d\n" % t for t in zip(r["x"], r["y"], r["inten"]))
    text += "\n".join(" ".join(repr(float(v)) for v in row) for row in want[::-1]) + "\n"
    path = tmp_path / "case.txt"
    path.write_text(text)
    r = subprocess.run([BIN, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
