"""Chain diagnostics on the device (include/flowstate.h 'Chain diagnostics') against the
float64 numpy restatement of tests/test_diagnostics_cpu.py: the autocovariance, tau and the
transition table bit for bit, the pooled sums within the bound of a float64 sum in any
order, the recorded row against the engine's own arrays and fs_classify_wells, and a recorded
run end to end.  All shapes are tiny; the restatement of each series is computed once."""
import functools
import json

import numpy as np
import pytest
import torch

from flowstate import _lib, analysis, diagnostics, io
from flowstate.MCMC import BatchedMonteCarlo, Physics
from test_diagnostics_cpu import (CONSTANT, EXCURSIONS, NONFINITE, TRUNCATED, ar1, autocov_ref, observe_ref, pool_truth,
                                  rhat_ref, sum_bound, tau_ref, transitions_ref, var_bound, wells_of)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0), (2, 1), (17, 7), (200, 199), (600, 512)]  # (T, W): the lag maximum, several tiles and lag blocks
CHAINS = [1, 63, 65, 130]  # under one wave, one wave and a tail, three workgroups with a tail


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _case(T, W, C):
    """A seeded normal series plus a per-chain drift, and its restatement."""
    rng = np.random.default_rng(1000 * T + C)
    x = rng.normal(0.0, 1.0, (T, C)) + 3.0 + 0.01 * np.arange(T)[:, None] * rng.normal(0.0, 1.0, C)
    return x, autocov_ref(x, W)


def _same(got, want, what):
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=what)


# ---------------------------------------------------------------- fs_chain_autocov
@pytest.mark.parametrize("T,W", SHAPES)
@pytest.mark.parametrize("C", CHAINS)
def test_autocov_is_the_restatement_bit_for_bit(C, T, W):
    x, (mean, acov) = _case(T, W, C)
    got_mean, got_acov = diagnostics.autocov(_cuda(x), W)
    _same(got_mean, mean, "mean")
    _same(got_acov, acov, "acov")


def test_autocov_on_a_strided_view():
    T, W, C = 200, 199, 65
    x, (mean, acov) = _case(T, W, C)
    buf = torch.full((T, C + 3), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :C] = _cuda(x)
    got_mean, got_acov = diagnostics.autocov(buf[:, :C], W)
    _same(got_mean, mean, "mean")
    _same(got_acov, acov, "acov")


def test_autocov_of_bytes():
    rng = np.random.default_rng(7)
    x = (rng.random((150, 70)) < 0.3).astype(np.uint8)
    x[:, 0], x[:, 1] = 1, 0  # constant indicator chains
    x[:, 2] = rng.integers(0, 256, 150)  # the whole byte range
    mean, acov = autocov_ref(x, 140)
    got_mean, got_acov = diagnostics.autocov(_cuda(x), 140)
    _same(got_mean, mean, "mean")
    _same(got_acov, acov, "acov")
    assert (acov[:, :2] == 0).all() and mean[0] == 1 and mean[1] == 0


def test_autocov_constant_and_nonfinite_chains():
    T, W, C = 80, 79, 66
    x = _case(200, 199, 130)[0][:T, :C].copy()
    x[:, 3] = 0.1  # a constant chain: mean 0.1 exactly, acov +0
    x[:, 64] = 0.1
    x[17, 5] = np.inf  # a +inf row
    x[79, 65] = np.inf  # in the last row and the second workgroup
    x[0, 7] = np.nan
    mean, acov = autocov_ref(x, W)
    got_mean, got_acov = diagnostics.autocov(_cuda(x), W)
    _same(got_mean, mean, "mean")  # NaN / inf exactly where the restatement has them
    _same(got_acov, acov, "acov")
    g = got_acov.cpu().numpy()
    assert got_mean[3].item() == 0.1 and (g[:, 3] == 0).all() and not np.signbit(g[:, [3, 64]]).any()
    assert got_mean[5].item() == np.inf and np.isnan(g[0, 5]) and np.isnan(g[0, 7])
    # T = 3 of the issue: (0.1 + 0.1 + 0.1) / 3 is not 0.1
    m3, a3 = diagnostics.autocov(torch.full((3, 1), 0.1, dtype=torch.float64, device="cuda"), 2)
    assert m3.item() == 0.1 and (a3 == 0).all()


@pytest.mark.parametrize("T,W", [(600, 513), (40, 40), (1, 1)])
def test_autocov_refuses_lags_beyond_its_limits(T, W):
    C = 5
    x = torch.zeros((T, C), dtype=torch.float64, device="cuda")
    mean = torch.full((C,), -7.0, dtype=torch.float64, device="cuda")
    acov = torch.full((W + 1, C), -7.0, dtype=torch.float64, device="cuda")
    rc = _lib.load().fs_chain_autocov(_lib.ptr(x), 0, T, C, C, W, _lib.ptr(mean), _lib.ptr(acov), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1  # FS_EINVAL
    assert (mean == -7.0).all() and (acov == -7.0).all()
    with pytest.raises(_lib.FlowStateError):
        diagnostics.autocov(x, W)


# ---------------------------------------------------------------- fs_chain_tau
def _check_tau(mean, acov, c=5.0):
    tau, window, flags = tau_ref(mean, acov, c)
    g_tau, g_window, g_flags = diagnostics.tau_window(_cuda(np.asarray(mean, np.float64)), _cuda(acov), c)
    _same(g_tau, tau, "tau")
    _same(g_window, window, "window")
    _same(g_flags, flags, "flags")
    return tau, window, flags


@pytest.mark.parametrize("T,W,C", [(200, 199, 130), (600, 512, 65), (17, 7, 63), (1, 0, 1)])
def test_tau_of_the_autocovariances_above(T, W, C):
    mean, acov = _case(T, W, C)[1]
    _check_tau(mean, acov)
    _check_tau(mean, acov, 1.5)


def test_tau_on_exact_ar1_and_one_chain_of_each_flag():
    W = 200
    acov = np.concatenate([ar1(0.0, W), ar1(0.5, W), ar1(0.9, W), ar1(0.999, W), np.zeros((W + 1, 1)),
                           np.full((W + 1, 1), np.nan), ar1(0.5, W)], axis=1)
    mean = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, np.inf])
    _, window, flags = _check_tau(mean, acov)
    assert list(flags) == [0, 0, 0, TRUNCATED, CONSTANT, NONFINITE, NONFINITE]
    assert window[3] == W and window[0] == 3
    _, _, flags = _check_tau(mean[2:3], ar1(0.9, 8))
    assert flags[0] == TRUNCATED


def test_tau_with_one_chain_on_a_pooled_curve():
    T, W, C = 200, 199, 130
    mean, acov = _case(T, W, C)[1]
    pooled, scalars = diagnostics.pool(_cuda(mean), _cuda(acov), T)
    p, s = pooled.cpu().numpy(), scalars.cpu().numpy()
    tau, window, flags = tau_ref(s[:1], p[:, None])
    g = diagnostics.tau_window(scalars[:1], pooled[:, None])
    _same(g[0], tau, "tau")
    _same(g[1], window, "window")
    _same(g[2], flags, "flags")


# ---------------------------------------------------------------- fs_chain_pool
@pytest.mark.parametrize("C,bad", [(1, 0), (2, 0), (2, 1), (257, 3), (1000, 5)])
def test_pool_against_fsum(C, bad):
    """Every plain sum of n terms is held to (n + 16) u sum |term| (test_diagnostics_cpu.sum_bound)
    and the variance of the means to the bound derived from that one in var_bound's docstring."""
    rng = np.random.default_rng(C + bad)
    T, W = 50, 6
    mean = rng.normal(3.0, 2.0, C)
    acov = rng.normal(0.0, 1.0, (W + 1, C))
    acov[0] = np.abs(acov[0]) + 0.1
    acov[0, C // 2] = 0.0  # a constant chain counts
    idx = rng.choice(C, bad, replace=False)
    for i, j in enumerate(idx):
        if i % 2:
            mean[j] = np.nan if i % 4 == 1 else np.inf
        else:
            acov[:, j] = np.nan
    t = pool_truth(mean, acov, T)
    n = t["n"]
    assert n == C - bad
    d_mean, d_acov = _cuda(mean), _cuda(acov)
    pooled, scalars = diagnostics.pool(d_mean, d_acov, T)
    again = diagnostics.pool(d_mean, d_acov, T)
    assert torch.equal(pooled, again[0]) and torch.equal(scalars, again[1])
    p, s = pooled.cpu().numpy(), scalars.cpu().numpy()
    assert s[3] == n  # exact with NaN chains present
    for k in range(W + 1):
        err, b = abs(p[k] - t["pooled"][k]), sum_bound(n, t["pooled_abs"][k]) / n
        print(f"pooled[{k}]: err {err:.3e} bound {b:.3e}")
        assert err <= b, k
    for name, got, want, b in (("grand mean", s[0], t["gm"], sum_bound(n, t["gm_abs"]) / n),
                               ("mean variance", s[2], t["mv"], sum_bound(n, t["mv_abs"]) / n),
                               ("variance of means", s[1], t["var"],
                                var_bound(n, t["var_s"], t["gm_abs"]) if n >= 2 else 0.0)):
        print(f"{name}: got {got!r} want {want!r} bound {b:.3e}")
        assert abs(got - want) <= b, name
    r = diagnostics.rhat_of(s.tolist(), T)
    want = rhat_ref(t["var"], t["mv"], n, T)
    assert (r is None) == (want is None) and (r is None or r == pytest.approx(want, rel=1e-12))


def test_pool_with_no_usable_chain_is_zero():
    mean = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    acov = torch.ones((4, 3), dtype=torch.float64, device="cuda")
    pooled, scalars = diagnostics.pool(mean, acov, 10)
    assert (pooled == 0).all() and (scalars == 0).all()


# ---------------------------------------------------------------- fs_chain_transitions
def test_transitions_on_random_series():
    rng = np.random.default_rng(11)
    N, C, T = 3, 130, 300
    n_a = rng.integers(0, N + 1, (T, C)).astype(np.uint8)
    n_b = (N - n_a) * (rng.random((T, C)) < 0.7)
    n_b = n_b.astype(np.uint8)
    want = transitions_ref(n_a, n_b, N)
    assert want[:, 3].sum() > C and want[:, 2].sum() > C  # hops and excursions do occur
    _same(diagnostics.transitions(_cuda(n_a), _cuda(n_b), N), want, "table")
    buf_a = torch.zeros((T, C + 5), dtype=torch.uint8, device="cuda")
    buf_b = torch.zeros_like(buf_a)
    buf_a[:, :C], buf_b[:, :C] = _cuda(n_a), _cuda(n_b)
    _same(diagnostics.transitions(buf_a[:, :C], buf_b[:, :C], N), want, "strided table")


def test_transitions_on_the_excursion_sequences():
    for states, want in EXCURSIONS.items():
        n_a, n_b = wells_of(states, 3)
        got = diagnostics.transitions(_cuda(n_a), _cuda(n_b), 3).cpu().numpy()
        assert tuple(got[0]) == want == tuple(transitions_ref(n_a, n_b, 3)[0]), states


# ---------------------------------------------------------------- fs_chain_observe
def _mixed_engine(N, C, seed):
    """An engine (no flow) whose odd chains hold float32 values and are flagged so, with
    particles scattered around both wells."""
    rng = np.random.default_rng(seed)
    L = float(np.sqrt(N / 0.03))
    centres = np.array([[L / 4, L / 2], [3 * L / 4, L / 2]])
    state = centres[rng.integers(0, 2, (C, N))] + rng.uniform(-1.2, 1.2, (C, N, 2))
    state[0], state[1] = centres[0] + rng.uniform(-0.5, 0.5, (N, 2)), centres[1] + rng.uniform(-0.5, 0.5, (N, 2))
    state[2], state[3] = state[0], state[1]
    f32 = (np.arange(C) % 2 == 1) | (np.arange(C) == 2)
    state[f32] = state[f32].astype(np.float32)
    bmc = BatchedMonteCarlo(None, state, Physics(L, L), np.arange(1, C + 1, dtype=np.uint64), device="cuda")
    bmc.state_is_f32.copy_(_cuda(f32.astype(np.uint8)))
    bmc.accept.copy_(_cuda((rng.random(C) < 0.4).astype(np.uint8)))
    bmc.W_old.copy_(_cuda(rng.normal(0, 5, C)))
    bmc.E_old.copy_(_cuda(rng.normal(-20, 5, C)))
    return bmc, f32


@pytest.mark.parametrize("N", [3, 16, 64])
def test_observe_writes_one_row_of_the_live_state(N):
    C, cap, t = 130, 4, 2
    bmc, f32 = _mixed_engine(N, C, N)
    rec = diagnostics.ChainRecorder(bmc, cap)
    for k, v in rec._buf.items():
        v.fill_(7 if v.dtype == torch.uint8 else -7.0)
    engine = {k: getattr(bmc, k).clone() for k in ("state", "state_is_f32", "E_old", "W_old", "accept", "pcg",
                                                    "attempts", "accepted", "nll_old")}
    rec.t = t
    rec.record()
    assert rec.t == t + 1
    rows = {k: v.cpu().numpy() for k, v in rec._buf.items()}
    for k, v in rows.items():  # every other row keeps the sentinel
        assert (np.delete(v, t, axis=0) == (7 if v.dtype == np.uint8 else -7.0)).all(), k
    for k, v in engine.items():
        assert torch.equal(getattr(bmc, k), v), k
    np.testing.assert_array_equal(rows["E"][t], engine["E_old"].cpu().numpy())
    np.testing.assert_array_equal(rows["W"][t], engine["W_old"].cpu().numpy())
    np.testing.assert_array_equal(rows["accept"][t], engine["accept"].cpu().numpy())
    # fs_classify_wells on the float32 cast of the float32 chains and on the float64 chains
    sel = _cuda(f32)
    for mask, dtype in ((sel, torch.float32), (~sel, torch.float64)):
        cls, _, avg_x = analysis.classify_wells(bmc.state[mask].to(dtype).contiguous(), bmc.phys.half_width,
                                                bmc.phys.r0)
        m = mask.cpu().numpy()
        np.testing.assert_array_equal(rows["avg_x"][t][m], avg_x.cpu().numpy())
        np.testing.assert_array_equal(rows["n_a"][t][m], (cls == 0).sum(1).cpu().numpy())
        np.testing.assert_array_equal(rows["n_b"][t][m], (cls == 1).sum(1).cpu().numpy())
    avg_x, n_a, n_b = observe_ref(engine["state"].cpu().numpy(), f32, bmc.phys.half_width, bmc.phys.r0)
    np.testing.assert_array_equal(rows["avg_x"][t], avg_x)
    np.testing.assert_array_equal(rows["n_a"][t], n_a)
    np.testing.assert_array_equal(rows["n_b"][t], n_b)
    assert (n_a[[0, 2]] == N).all() and (n_b[[1, 3]] == N).all() and 0 < (n_a + n_b < N).sum()


def test_observe_skips_the_series_that_are_off():
    bmc, _ = _mixed_engine(3, 10, 1)
    rec = diagnostics.ChainRecorder(bmc, 2, observables=("E", "wells"))
    rec.record()
    s = rec.series()
    assert set(k for k, v in s.items() if torch.is_tensor(v)) == {"E", "n_a", "n_b"} and s["E"].shape == (1, 10)
    assert torch.equal(s["E"][0], bmc.E_old)
    with pytest.raises(ValueError):
        diagnostics.ChainRecorder(bmc, 2, observables=("E", "pressure"))


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def recorded_run():
    """The Algorithm-2 test flow (N = 3) on 130 chains, 40 steps one at a time: once recorded,
    once not."""
    from flowstate.MCMC.initialise import initialise_low_left, initialise_low_right
    from test_gpu_algorithm2 import _cycle_model

    C, steps = 130, 40
    m = _cycle_model().cuda().eval()
    B = float(m.flows[0].tail_bound)
    init = np.array([(initialise_low_left if i % 2 == 0 else initialise_low_right)(3, 0.03, 1.0)[0] for i in range(C)])

    def engine():
        return BatchedMonteCarlo(m, init, Physics(2 * B), [42 + i for i in range(C)], device="cuda")

    plain = engine()
    for _ in range(steps):
        plain.step(1)
    bmc = engine()
    rec = diagnostics.ChainRecorder(bmc, steps)
    diagnostics.record_steps(bmc, steps, rec)
    torch.cuda.synchronize()
    bmc.check_errors()
    return plain, bmc, rec


def test_recording_leaves_the_chains_unchanged(recorded_run):
    plain, bmc, rec = recorded_run
    for k in ("state", "pcg", "E_old", "nll_old", "attempts", "accepted"):
        assert torch.equal(getattr(plain, k), getattr(bmc, k)), k
    assert rec.t == 40
    s = rec.series()
    assert torch.equal(s["E"][-1], bmc.E_old) and torch.equal(s["accept"][-1], bmc.accept)
    assert int(s["accept"].sum()) == int(bmc.accepted.sum())
    with pytest.raises(RuntimeError, match="full"):
        rec.record()
    rec2 = diagnostics.ChainRecorder(bmc, 1)
    rec2.record()
    rec2.reset()
    rec2.record()
    assert rec2.t == 1


def test_diagnose_is_the_restatement_of_the_copied_series(recorded_run, tmp_path):
    _, bmc, rec = recorded_run
    res = diagnostics.diagnose(rec)
    s = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in rec.series().items()}
    T, C, N = 40, 130, 3
    W = T - 1
    assert res["summary"]["max_lag"] == W and res["summary"]["T"] == T
    series = dict(E=s["E"], avg_x=s["avg_x"], accept=s["accept"], in_a=(s["n_a"] == N).astype(np.uint8))
    for name, x in series.items():
        mean, acov = autocov_ref(x, W)
        tau, window, flags = tau_ref(mean, acov)
        pc, sm = res["per_chain"][name], res["summary"][name]
        _same(pc["mean"], mean, name)
        _same(pc["acov"], acov, name)
        _same(pc["tau"], tau, name)
        _same(pc["window"], window, name)
        _same(pc["flags"], flags, name)
        skip = (flags == CONSTANT) | (flags == NONFINITE)
        with np.errstate(divide="ignore"):
            _same(pc["ess"], np.where(skip, 0.0, T / (2.0 * np.where(skip, 1.0, tau))), name)
        t = pool_truth(mean, acov, T)
        n = t["n"]
        assert sm["n_used"] == n and sm["n_constant"] == int((flags == CONSTANT).sum())
        assert sm["n_truncated"] == int((flags == TRUNCATED).sum()) and sm["n_nonfinite"] == 0
        p = pc["pooled"].cpu().numpy()
        assert (np.abs(p - t["pooled"]) <= sum_bound(n, t["pooled_abs"]) / n).all(), name
        assert abs(sm["mean"] - t["gm"]) <= sum_bound(n, t["gm_abs"]) / n
        assert abs(sm["mean_var"] - t["mv"]) <= sum_bound(n, t["mv_abs"]) / n
        assert abs(sm["var_of_means"] - t["var"]) <= var_bound(n, t["var_s"], t["gm_abs"])
        tp, wp, fp = tau_ref([sm["mean"]], p[:, None])
        assert (sm["tau"], sm["window"], sm["flags"]) == (tp[0], wp[0], fp[0])
        assert sm["rhat"] == rhat_ref(sm["var_of_means"], sm["mean_var"], n, T)
        if fp[0] in (0, TRUNCATED):
            assert sm["ess_total"] == n * T / (2.0 * tp[0])
    np.testing.assert_array_equal(res["transitions"].cpu().numpy(), transitions_ref(s["n_a"], s["n_b"], N))
    tot = transitions_ref(s["n_a"], s["n_b"], N)[:, :5].sum(0)
    tr = res["summary"]["transitions"]
    assert (tr["steps_a"], tr["steps_b"], tr["steps_neither"], tr["hops_ab"], tr["hops_ba"]) == tuple(tot)
    assert tr["hop_rate"] == (tot[3] + tot[4]) / (T * C)
    assert tr["mean_residence"] == (tot[0] + tot[1]) / max(tot[3] + tot[4], 1)
    V = bmc.phys.box_x * bmc.phys.box_y
    assert res["summary"]["pressure_mean"] == pytest.approx(N / V / bmc.phys.beta + s["W"].mean() / (2 * V), rel=1e-12)
    path = io.write_chain_diagnostics(str(tmp_path), res)
    assert path.endswith("chain_diagnostics_data.json")
    back = json.load(open(path))
    assert back == res["summary"]
    assert diagnostics.diagnose(rec.series(), max_lag=10)["summary"]["max_lag"] == 10
