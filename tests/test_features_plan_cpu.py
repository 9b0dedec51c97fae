"""The build table and the launch plan of the metric kernel (nyxus_amd/csrc/features_plan.h) as a stand-alone program, plain and under
the address and undefined-behaviour sanitizers: the plan against a transcription of the selection chain the launcher had before the
table, on the full grid of its inputs; the table's coverage; the literal rows of the benchmark configuration (tests/cpp/test_features_plan.cpp).
The program has its own main and walks the grid on the machine's cores; nothing is preloaded."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_features_plan.cpp")
HDR = os.path.join(ROOT, "nyxus_amd", "csrc", "features_plan.h")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_features_plan_program(tmp_path, flags):
    exe = str(tmp_path / "test_features_plan.bin")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", *flags, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    m = re.search(r"plan == oracle on (\d+) grid points", r.stdout)
    assert m and int(m.group(1)) == 3 * 2 * 2 * 2 * 2 * 2 * 6 * 9 * 2 * 3 * 3 * 2 * 2 * 7 * 2 * 2 * 3 * 2 * 3 * 2 * 6, r.stdout
    assert "benchmark: tier 8, FAM 1, WIN 0, deferred" in r.stdout and "g16w8" in r.stdout and "workspace" in r.stdout


def test_the_plan_header_is_plain_and_blind_to_the_environment():
    src = open(HDR).read()
    assert "getenv" not in src and "hip/" not in src and "knobs.h" not in src
