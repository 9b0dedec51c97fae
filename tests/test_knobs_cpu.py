"""The register of NYXHIP_* environment knobs (nyxus_amd/csrc/knobs.h) on the host: a stand-alone program (tests/cpp/test_knobs.cpp)
that includes the header with plain g++ -- no HIP, no library -- built once as it is and once under the address and
undefined-behaviour sanitizers.  The per-process knobs are read once, so every start-up environment is a fresh child process.
Source level: the table, INTEGRATION.md section 4 and the translation units agree on what knobs exist and who reads the environment."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_knobs.cpp")
CSRC = os.path.join(ROOT, "nyxus_amd", "csrc")
PER_CALL = {"NYXHIP_" + n for n in ("DEBUG", "DEP_SEQ", "G16_FUSED", "NO_COOP_GABOR", "MAX_OCC", "LARGE_BUDGET_MB", "LARGE_DBG")}


@pytest.fixture(scope="module", params=[["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("knobs") / "test_knobs.bin")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *request.param, SRC, "-o", out], check=True, capture_output=True, text=True)
    return out


def run(exe, *args, **env):
    """The program in a child process whose only NYXHIP_* variables are `env`."""
    base = {k: v for k, v in os.environ.items() if not k.startswith("NYXHIP_")}
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=dict(base, **{"NYXHIP_" + k: v for k, v in env.items()}))
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    return r.stdout


def start(exe, **env):
    """accessor -> value as a process started in `env` reads it."""
    return {k: int(v) for k, v in (line.split() for line in run(exe, "--start", **env).splitlines())}


def table(exe):
    return [line.split() for line in run(exe, "--list").splitlines()]


def test_knobs_program(exe):
    assert "ALL PASSED" in run(exe)


@pytest.mark.parametrize("value,on", [(None, 0), ("", 0), ("0", 0), ("00", 0), ("01", 0), ("1", 1), ("yes", 1)])
def test_flag_rule_of_a_per_process_flag(exe, value, on):
    got = start(exe, **({} if value is None else {"NO_SMALL": value, "STAMPS": value, "GABOR_NO_LPSEP": value}))
    assert (got["no_small"], got["stamps"], got["gabor_no_lpsep"]) == (on, on, on)


def test_per_process_integers(exe):
    dflt = dict(g16_w8_min=2304, mom_occ=6, tex_occ=8, dbg_phase=0, gabor_mode_env=4)
    unset, empty = start(exe), start(exe, G16_W8_MIN="", MOM_OCC="", TEX_OCC="", DBG_PHASE="", GABOR_MODE="")
    given = start(exe, G16_W8_MIN="1024", MOM_OCC="4", TEX_OCC="7", DBG_PHASE="6", GABOR_MODE="3")
    for k, v in dflt.items():
        assert unset[k] == v and empty[k] == v, k
    assert [given[k] for k in dflt] == [1024, 4, 7, 6, 3]


@pytest.mark.parametrize("env,mode", [({}, 4), ({"GABOR_MODE": "2"}, 2), ({"GABOR_MODE": "3"}, 3), ({"GABOR_MODE": "5"}, 4), ({"GABOR_EXACT": "1"}, 0),
                                      ({"GABOR_EXACT": "1", "GABOR_MODE": "2"}, 0), ({"GABOR_FUSED": "1"}, 1),
                                      ({"GABOR_FUSED": "1", "GABOR_EXACT": "1", "GABOR_MODE": "3"}, 1), ({"GABOR_FUSED": "0", "GABOR_EXACT": "1"}, 0),
                                      ({"GABOR_FUSED": "0", "GABOR_EXACT": "", "GABOR_MODE": "2"}, 2)])
def test_gabor_mode_precedence(exe, env, mode):
    assert start(exe, **env)["gabor_mode"] == mode


@pytest.mark.parametrize("env,off", [({}, 0), ({"NO_COOP_TEX_SC2": "1"}, 1), ({"NO_COOP_TEX": "1"}, 1), ({"NO_COOP": "1"}, 1),
                                     ({"NO_COOP_TEX_SC2": "0", "NO_COOP_TEX": "", "NO_COOP": "0"}, 0)])
def test_no_sc2_tex_sources(exe, env, off):
    assert start(exe, **env)["no_sc2_tex"] == off


def test_table_is_the_documented_set(exe):
    """Every row is in the table of INTEGRATION.md section 4 and the other way round (NYXHIP_LIB is read by the Python side only)."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("\n## 4. "):]
    section = section[:section.index("\n## ", 1)] if "\n## " in section[1:] else section
    documented = set()
    for line in section.splitlines():
        if line.startswith("| `NYXHIP_"):
            documented |= set(re.findall(r"NYXHIP_[A-Z0-9_]+", line.split("|")[1]))
    rows = [r[0] for r in table(exe)]
    assert len(rows) == len(set(rows)) == 37
    assert set(rows) == documented - {"NYXHIP_LIB"}, sorted(set(rows) ^ (documented - {"NYXHIP_LIB"}))


def test_per_call_rows(exe):
    rows = table(exe)
    assert {name for name, _, when in rows if when == "call"} == PER_CALL
    assert all(when in ("call", "process") and kind in ("flag", "integer") for _, kind, when in rows)


def test_one_file_reads_the_environment():
    readers = [f for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f)) and "getenv" in open(os.path.join(CSRC, f), errors="replace").read()]
    assert readers == ["knobs.h"]
