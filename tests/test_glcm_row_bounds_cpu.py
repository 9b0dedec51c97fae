"""The row blocks of the co-occurrence sweep (nyxus_amd/csrc/roi_kernel.h: glcm_row_bounds, glcm_row_bounds_even) on the host: a
stand-alone program (tests/cpp/test_glcm_row_bounds.cpp) that includes the header with plain g++ -- no HIP, no library -- and walks
every box height 1 .. 8192; built and run once as it is and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_glcm_row_bounds.cpp")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_glcm_row_bounds_program(tmp_path, flags):
    exe = str(tmp_path / "test_glcm_row_bounds.bin")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert "ok   glcm_row_bounds: heights 1 .. 8192" in r.stdout and "ok   glcm_row_bounds_even: heights 1 .. 8192" in r.stdout
