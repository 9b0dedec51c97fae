"""RadialDistributionFeature of the C++ plugin adapter (include/nyxhip_feature_method.hpp): compiles on the CPU; on the GPU the
reference-style unit test (tests/cpp/test_radial_method.cpp) reproduces the reference's regression vector for the shape2d ROI."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_radial_method.bin")


def _build():
    lib = os.path.join(ROOT, "nyxus_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "test_radial_method.cpp"),
           "-o", BIN, "-L", lib, "-lnyxhip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_radial_adapter_compiles_and_links_against_the_abi():
    _build()
    r = subprocess.run([BIN, "--compile-check"], capture_output=True, text=True)
    assert r.returncode == 0 and "compiled" in r.stdout


@pytest.mark.gpu
def test_reference_style_radial_test_passes_on_gpu(tmp_path):
    if not os.path.exists(BIN):
        _build()
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_tests.json")))
    reg = json.load(open(os.path.join(ROOT, "tests", "golden", "radial", "reference_regression.json")))
    px = [t for t, m in zip(ref["pixels"]["shape2d_morphology_intensity"], ref["pixels"]["shape2d_morphology_mask"]) if m[2] != 0]
    want = reg["FRAC_AT_D"] + reg["MEAN_FRAC"] + reg["RADIAL_CV"]
    path = tmp_path / "case.txt"
    path.write_text("%d\n" % len(px) + "".join("%d %d %d\n" % tuple(t) for t in px) + "\n".join(repr(v) for v in want) + "\n")
    r = subprocess.run([BIN, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
