"""bench.py's launch contract on the CPU: `--gpus N` never prints a single-rank line.
With WORLD_SIZE set by a launcher it must equal --gpus; without one, bench.py starts
the N rank processes itself (torch.distributed.run as a child) and exits with their
code.  Here there is no GPU, so the ranks fail and the exit code is non-zero, with no
JSON line on stdout."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra, drop=()):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=240)


def test_algorithm1_regime_cpu_sample_is_bounded():
    """The regime leg's CPU sample (the reference's per-call numpy local moves,
    oracle.physics.NumpyLocalChain, + torch-CPU log_prob) runs at least one attempt, stops
    near its budget and reports itself as a port of the reference's loop."""
    import time
    import bench
    t0 = time.perf_counter()
    r = bench.algorithm1_regime_cpu(N=3, interval=50, budget_s=0.3)
    # (the A1 flow's construction and 64 untimed CPU proposals dominate: ~2 s alone, more
    # when the suite runs in parallel workers)
    assert time.perf_counter() - t0 < 120
    assert r["value"] > 0 and r["kind"] == "port" and r["unit"] == "big-move attempts/s"
    assert r["cores"] >= 1 and "attempts of one run" in r["sample"] and "numpy" in r["sample"]


def test_dump_outputs_at_headline_size_is_a_fixed_sample_within_64mb(tmp_path):
    """--dump-outputs at the headline's 65536 chains (the tensors a step leaves, here on
    the CPU): float32 / float64 .npy files, 64 MB at the most in all, the per-chain values
    of every chain and the (C, 2N) arrays for one fixed, seeded sample of chains."""
    import types

    import numpy as np
    import torch

    import bench

    C, N = 65536, 64
    g = torch.Generator().manual_seed(3)
    r = lambda *s, dt=torch.float64: torch.rand(*s, generator=g, dtype=dt)  # noqa: E731
    st = types.SimpleNamespace(config=r(C, 2 * N, dt=torch.float32), centered=r(C, 2 * N, dt=torch.float32),
                               log_q=r(C, dt=torch.float32), E_new=r(C), W_new=r(C))
    bmc = types.SimpleNamespace(C=C, N=N, device=torch.device("cpu"), state=r(C, N, 2), E_old=r(C), W_old=r(C),
                                nll_old=r(C), accept=(r(C) < 0.5).to(torch.uint8),
                                accepted=torch.arange(C), attempts=torch.arange(C) + 1)
    st.E_new[::3] = float("inf")  # overlapping proposals
    st.W_new[::3] = float("inf")
    st.E_new[1], st.E_new[2] = float("-inf"), float("nan")
    red = (torch.ones(99, 99, dtype=torch.int64), torch.tensor([1, 2, C]), torch.ones(C, 3, dtype=torch.int64))
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bmc, st, red, 0, 1)
        got.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = got
    assert all(f.endswith(".npy") for f in os.listdir(tmp_path / "a"))
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    rows = a["rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_ROWS and len(np.unique(rows)) == len(rows) and (np.diff(rows) > 0).all()
    assert (a["rows"] == b["rows"]).all()
    assert (a["proposal"] == st.config.numpy()[rows]).all() and a["proposal"].dtype == np.float32
    assert (a["proposal_centered"] == st.centered.numpy()[rows]).all()
    assert (a["state"] == bmc.state.numpy().reshape(C, -1)[rows]).all()
    # finite files only: a non-finite value is written as 0, its kind beside it
    assert all(np.isfinite(v).all() for v in a.values())
    assert sorted(k for k in a if k.endswith("_nonfinite")) == ["E_new_nonfinite", "W_new_nonfinite", "log_q_nonfinite"]
    kind = np.zeros(C, np.float32)
    kind[::3], kind[1], kind[2] = 1, 2, 3
    assert (a["E_new_nonfinite"] == kind).all() and not a["log_q_nonfinite"].any()
    assert (a["W_new_nonfinite"] == (np.arange(C) % 3 == 0)).all()
    st.E_new = torch.where(torch.from_numpy(kind) == 0, st.E_new, 0.0)
    st.W_new = torch.where(torch.isfinite(st.W_new), st.W_new, 0.0)
    for k, t in (("log_q", st.log_q), ("E_new", st.E_new), ("W_new", st.W_new), ("E_old", bmc.E_old),
                 ("W_old", bmc.W_old), ("nll_old", bmc.nll_old), ("accept", bmc.accept), ("accepted", bmc.accepted),
                 ("attempts", bmc.attempts)):
        assert a[k].shape == (C,) and (a[k] == t.numpy()).all(), k
    assert a["hist"].shape == (99, 99) and (a["wells"] == [1, 2, C]).all() and a["chain_counters"].shape == (C, 3)


def test_steps_must_be_positive():
    r = _bench(["--gpus", "1", "--steps", "0"], {})
    assert r.returncode == 2 and "--steps" in r.stderr
    assert '"metric"' not in r.stdout


def test_world_size_must_match_gpus():
    r = _bench(["--gpus", "2"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2, r.stderr[-2000:]
    assert "--gpus 2 but WORLD_SIZE=1" in r.stderr
    assert '"metric"' not in r.stdout


def test_gpus_without_launcher_spawns_ranks():
    r = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], {},
               drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"))
    assert r.returncode != 0
    assert '"metric"' not in r.stdout
    # the ranks were started by torch.distributed.run (its own banner / error report)
    assert "torch.distributed" in r.stderr or "ChildFailedError" in r.stderr or "2 ranks need 2 GPUs" in r.stderr, \
        r.stderr[-2000:]
