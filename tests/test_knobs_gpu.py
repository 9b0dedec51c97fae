"""GPU test: the knobs that nyxus_amd/csrc/knobs.h marks `call` are read on every call, on a live context -- the shared session
context here, between calls that other tests have long since made.  NYXHIP_DEBUG makes roi_dependence's launch report its layout on
stderr ("... par 1": the three feature tails side by side; "par 0": one after the other, what NYXHIP_DEP_SEQ asks for)."""
import numpy as np
import pytest

from nyxus_amd import _abi

pytestmark = pytest.mark.gpu

MASK = _abi.FAM_GLDZM | _abi.FAM_GLDM | _abi.FAM_NGLDM


def test_per_call_knobs_follow_the_environment_between_calls(hip_ctx, capfd, monkeypatch):
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:12, 0:12]
    rois = [dict(x=xx.ravel().astype(np.int64), y=yy.ravel().astype(np.int64), inten=rng.integers(1, 4096, 144).astype(np.uint32)) for _ in range(4)]
    b = _abi.batch_from_rois(rois)
    s = _abi.default_settings(8)

    def call():
        """The table, and what the dependence launches of the call said on stderr: their `par` values and every [nyxhip] line."""
        capfd.readouterr()
        table = hip_ctx.featurize_host(b, MASK, s)
        lines = [line for line in capfd.readouterr().err.splitlines() if "[nyxhip]" in line]
        return table, [line.rsplit(" ", 2)[-2:] for line in lines if "dependence launch" in line], lines

    for k in ("NYXHIP_DEBUG", "NYXHIP_DEP_SEQ"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NYXHIP_DEBUG", "1")
    par, said, _ = call()
    assert said and all(w == ["par", "1"] for w in said), said
    monkeypatch.setenv("NYXHIP_DEP_SEQ", "1")
    seq, said, _ = call()
    assert said and all(w == ["par", "0"] for w in said), said
    assert np.array_equal(par.view(np.uint64), seq.view(np.uint64))
    monkeypatch.delenv("NYXHIP_DEP_SEQ")
    again, said, _ = call()
    assert said and all(w == ["par", "1"] for w in said), said
    monkeypatch.setenv("NYXHIP_DEP_SEQ", "0")                 # one flag rule: "0" is off
    _, said, _ = call()
    assert said and all(w == ["par", "1"] for w in said), said
    monkeypatch.delenv("NYXHIP_DEBUG")
    quiet, _, lines = call()
    assert not lines, lines
    assert np.array_equal(par.view(np.uint64), again.view(np.uint64)) and np.array_equal(par.view(np.uint64), quiet.view(np.uint64))
