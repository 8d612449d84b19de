"""bench.py's plain run on the GPU, in process at a small size (the headline's flow and
kernels, N=64, 4096 chains): the result line holds the headline fields and none of the
--full legs, --steps sets the number of timed steps, and --dump-outputs writes the last
timed step's outputs, identical from run to run with the same arguments."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FULL_LEGS = ("acceptance_match", "alt_precision", "single_pass", "given_proposal", "config2", "config5",
             "algorithm1_regime", "cpu_baseline", "vs_cpu_baseline")


def _run(monkeypatch, capsys, out_dir, steps):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                                      "--chains", "4096", "--dump-outputs", str(out_dir)])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_plain_run_is_lean_and_dumps_reproducible_outputs(monkeypatch, capsys, tmp_path):
    C, D = 4096, 128
    r1, d1 = _run(monkeypatch, capsys, tmp_path / "a", 2)
    r2, d2 = _run(monkeypatch, capsys, tmp_path / "b", 2)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r1
    assert r1["steps"] == 2 and r1["unit"] == "steps/s" and r1["dtype"] == "f32" and r1["higher_is_better"] is True
    assert r1["ms_per_step"] > 0 and abs(r1["value"] - C / (r1["ms_per_step"] * 1e-3)) <= 1e-6 * r1["value"]
    assert not [k for k in FULL_LEGS if k in r1] and r1["parity_checked"] is None
    # the arrays a caller of the timed path receives, float32 / float64, all finite where
    # the step defines them
    assert set(d1) == {"rows", "proposal", "proposal_centered", "log_q", "E_new", "W_new", "accept", "state",
                       "E_old", "W_old", "nll_old", "accepted", "attempts", "hist", "wells", "chain_counters",
                       "log_q_nonfinite", "E_new_nonfinite", "W_new_nonfinite"}  # no other array needed coding
    assert all(a.dtype in (np.float32, np.float64) for a in d1.values())
    # every file finite; an overlapping proposal's infinite energy is coded beside it, and
    # no such proposal was accepted
    assert all(np.isfinite(a).all() for a in d1.values())
    for k in ("log_q", "E_new", "W_new"):
        assert d1[k + "_nonfinite"].shape == (C,) and set(np.unique(d1[k + "_nonfinite"])) <= {0.0, 1.0, 2.0, 3.0}
    assert (d1["E_new"][d1["E_new_nonfinite"] != 0] == 0).all()
    assert not ((d1["E_new_nonfinite"] != 0) & (d1["accept"] == 1)).any()
    assert sum(a.nbytes for a in d1.values()) <= 64 << 20
    assert d1["proposal"].shape == (C, D) and d1["state"].shape == (C, D) and d1["log_q"].shape == (C,)
    assert (d1["rows"] == np.arange(C)).all()
    assert set(np.unique(d1["accept"])) <= {0.0, 1.0}
    # the accepted proposals of the last step are the chains' states
    acc = d1["accept"] == 1
    assert (d1["state"][acc] == d1["proposal"][acc].astype(np.float64)).all()
    assert (d1["E_old"][acc] == d1["E_new"][acc]).all()
    # same arguments, same inputs, same outputs
    assert d1.keys() == d2.keys()
    for k in d1:
        assert np.array_equal(d1[k], d2[k], equal_nan=True), k
    # --steps sets the timed steps: one more step, one more attempt per chain
    r3, d3 = _run(monkeypatch, capsys, tmp_path / "c", 3)
    assert r3["steps"] == 3 and (d3["attempts"] == d1["attempts"] + 1).all()
