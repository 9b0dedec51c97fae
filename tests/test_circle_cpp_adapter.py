"""EnclosingInscribingCircumscribingCircleFeature and GeodeticLengthThicknessFeature of the C++ plugin adapter
(include/nyxhip_feature_method.hpp): compiles on the CPU; on the GPU the reference-style unit test (tests/cpp/test_circle_method.cpp)
reproduces the values recorded from the reference's classes for one ROI of tests/circle_cases.py at its absolute position."""
import os
import subprocess

import pytest

from tests import circle_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_circle_method.bin")


def _build():
    lib = os.path.join(ROOT, "nyxus_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "test_circle_method.cpp"),
           "-o", BIN, "-L", lib, "-lnyxhip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_circle_adapter_compiles_and_links_against_the_abi():
    _build()
    r = subprocess.run([BIN, "--compile-check"], capture_output=True, text=True)
    assert r.returncode == 0 and "compiled" in r.stdout


@pytest.mark.gpu
def test_reference_style_circle_test_passes_on_gpu(tmp_path):
    if not os.path.exists(BIN):
        _build()
    k = circle_cases.N_PLACED + 6                        # the plate with a hole at (4093, 60001): a merged multicontour, absolute coordinates
    roi = circle_cases.placed()[k]
    G = circle_cases.golden()["placed"]
    want = G["table"][k, :5]
    assert G["n_contour"][k] > 100 and (want > 0).all()
    path = tmp_path / "case.txt"
    path.write_text("%d\n" % len(roi["x"]) + "".join("%d %d %d\n" % (x, y, v) for x, y, v in zip(roi["x"], roi["y"], roi["inten"]))
                    + "\n".join(repr(float(v)) for v in want) + "\n")
    r = subprocess.run([BIN, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
