"""IntensityHistogramFeatures of the C++ plugin adapter (include/nyxhip_feature_method.hpp): compiles on the CPU; on the GPU the
reference-style unit test (tests/cpp/test_ih_method.cpp) reproduces the values recorded from the reference's class for the ROIs of
tests/ih_cases.py's "sizes" case through runParallel(IntensityHistogramFeatures::reduce, ...)."""
import os
import subprocess

import pytest

from tests import ih_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_ih_method.bin")


def _build():
    lib = os.path.join(ROOT, "nyxus_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "test_ih_method.cpp"),
           "-o", BIN, "-L", lib, "-lnyxhip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_ih_adapter_compiles_and_links_against_the_abi():
    _build()
    r = subprocess.run([BIN, "--compile-check"], capture_output=True, text=True)
    assert r.returncode == 0 and "compiled" in r.stdout


@pytest.mark.gpu
def test_reference_style_ih_test_passes_on_gpu(tmp_path):
    if not os.path.exists(BIN):
        _build()
    name = "sizes"                                       # 63 .. 257 px and a 700-px ROI: both launch forms
    rois = ih_cases.CASES[name]["rois"]()
    s = ih_cases.settings(name)
    want = ih_cases.golden()[name]["table"]
    assert len(rois) == len(want) == 7
    text = "%d %r %d\n" % (s.grey_depth, -7777.0, len(rois))
    for k, r in enumerate(rois):
        text += "%d %d\n" % (k + 1, len(r["x"])) + "".join("%d %d %d\n" % t for t in zip(r["x"], r["y"], r["inten"]))
    text += "\n".join(" ".join(repr(float(v)) for v in row) for row in want) + "\n"
    path = tmp_path / "case.txt"
    path.write_text(text)
    r = subprocess.run([BIN, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
