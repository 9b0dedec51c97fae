"""The chunk arithmetic of the deferred-list launches (nyxus_amd/csrc/deferred_list.h: deferred_chunk) on the host: a stand-alone
program (tests/cpp/test_deferred_chunk.cpp) that includes the header with plain g++ -- no HIP, no library -- and walks the chunk
loop; built and run once as it is and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_deferred_chunk.cpp")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_deferred_chunk_program(tmp_path, flags):
    exe = str(tmp_path / "test_deferred_chunk.bin")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert "stride 0 is reported" in r.stdout
