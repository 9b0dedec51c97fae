"""The workspace arithmetic of the volume entries (nyxus_amd/csrc/vol_plan.h: vol_chunk, vol_sides, the *_layout functions) on the
host: a stand-alone program (tests/cpp/test_vol_plan.cpp) that includes the header with plain g++ -- no HIP, no library -- and holds
the chunk counts, the side fold and every entry's strides and bytes per ROI to literal numbers; built and run once as it is and once
under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_vol_plan.cpp")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_vol_plan_program(tmp_path, flags):
    exe = str(tmp_path / "test_vol_plan.bin")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert "per_roi 0 is not divided by" in r.stdout
