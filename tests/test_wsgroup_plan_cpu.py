"""The host plan of nyxhip_wsgroup_slides (nyxus_amd/csrc/wsgroup_plan.h) as a stand-alone program, plain and under the address and
undefined-behaviour sanitizers (tests/cpp/test_wsgroup_plan.cpp): the band cut on the full grid of small shapes and at sides 1 and 65534,
the workspace, and budgets that give one chunk, two chunks and a shorter last chunk.  The program has its own main; nothing is preloaded."""
import os
import re
import subprocess

import pytest

from nyxus_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_wsgroup_plan.cpp")
HDR = os.path.join(ROOT, "nyxus_amd", "csrc", "wsgroup_plan.h")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_wsgroup_plan_program(tmp_path, flags):
    exe = str(tmp_path / "test_wsgroup_plan.bin")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    m = re.search(r"band cut checked on (\d+) shapes", r.stdout)
    assert m and int(m.group(1)) == 300 * 300 + 15 * 15, r.stdout


def test_the_plan_header_is_plain_and_the_mirror_agrees():
    src = open(HDR).read()
    assert "getenv" not in src and "hip/" not in src
    m = re.search(r"constexpr uint32_t WS_BAND_PIXELS = (\d+);", src)
    assert m and int(m.group(1)) == _abi.WS_BAND_PIXELS
