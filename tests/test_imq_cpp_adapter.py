"""FocusScoreFeature and SaturationFeature of the C++ plugin adapter (include/nyxhip_feature_method.hpp): compiles on the CPU; on the GPU the
reference-style unit test (tests/cpp/test_imq_method.cpp) reproduces the values recorded from the reference's classes for the ROIs of
tests/imq_cases.py's "filled", "shapes" and "widths" cases through runParallel(F::parallel_process_1_batch, ...) and
reduce_trivial_rois_manual()."""
import os
import subprocess

import numpy as np
import pytest

from tests import imq_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_imq_method.bin")


def _build():
    lib = os.path.join(ROOT, "nyxus_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "test_imq_method.cpp"),
           "-o", BIN, "-L", lib, "-lnyxhip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_imq_adapter_compiles_and_links_against_the_abi():
    _build()
    r = subprocess.run([BIN, "--compile-check"], capture_output=True, text=True)
    assert r.returncode == 0 and "compiled" in r.stdout


@pytest.mark.gpu
def test_reference_style_imq_test_passes_on_gpu(tmp_path):
    if not os.path.exists(BIN):
        _build()
    names = ("filled", "shapes", "widths")               # even and odd sides, background cells, boxes about a wave wide
    rois = [r for n in names for r in imq_cases.CASES[n]()]
    want = np.concatenate([imq_cases.golden()[n] for n in names])
    assert len(rois) == len(want) == 13
    text = "%r %d\n" % (imq_cases.SOFT_NAN, len(rois))
    for k, r in enumerate(rois):
        text += "%d %d\n" % (k + 1, len(r["x"])) + "".join("%d %d %d\n" % t for t in zip(r["x"], r["y"], r["inten"]))
    text += "\n".join(" ".join(repr(float(v)) for v in row) for row in want) + "\n"
    path = tmp_path / "case.txt"
    path.write_text(text)
    r = subprocess.run([BIN, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
