"""Importance weights of flow samples on the device (fs_importance_weights,
fs_weighted_reduce, fs_weighted_hist2d, analysis.sample_analysis(reweight=...),
Algorithm2(reweight_analysis=True)) against the float64 numpy restatement of
tests/test_importance_cpu.py.

Tolerances are derived, not tuned (test_importance_cpu.bound): with u = 2^-53, n rows and
spread the distance between the largest and smallest finite log-weight, a float64 sum of
the n non-negative terms exp(lw - shift) in any order is within (n + 4 spread + 16) u
relative of the exact sum; S2 takes twice that, ess four times, hist_w and every *_w
output twice.  sum_lw, a sum of signed terms, takes the bound relative to sum |lw|.  The
truth is math.fsum over numpy.exp with the global maximum as shift."""
import json
import math
import os

import numpy as np
import pytest
import torch

from flowstate import _lib, analysis
from flowstate.MCMC import BatchedMonteCarlo, Physics
from flowstate.MCMC.energy_calculator import total_energy
from test_importance_cpu import U, Stream, bound, log_weights, normalised, truth, weighted_hist

pytestmark = pytest.mark.gpu


def _half_box(N):
    return ((N / 0.03) ** (1 / 2)) / 2


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _weights(state, beta, E, log_q):
    """One fs_importance_weights call -> log_w (numpy)."""
    E, q = _cuda(np.asarray(E, np.float64)), _cuda(np.asarray(log_q, np.float32))
    lw = torch.full((E.numel(),), 7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().fs_importance_weights(beta, E.numel(), _lib.ptr(E), _lib.ptr(q), _lib.ptr(lw),
                                                 _lib.ptr(state), _lib.stream_ptr()), "fs_importance_weights")
    return lw


def _check_header(h, lw_all, n_zero, n_bad):
    """The seven statistics against the truth over all rows seen."""
    mx, s1, s2, sl, sabs = truth(lw_all)
    b = bound(lw_all)
    got_mx, got_s1, got_s2, got_sl, n, nz, nb = h
    print(f"n={n} bound={b:.3e} S1 {abs(got_s1 - s1) / max(s1, 1e-300):.3e} S2 {abs(got_s2 - s2) / max(s2, 1e-300):.3e} "
          f"sum_lw {abs(got_sl - sl) / max(sabs, 1e-300):.3e}")
    assert got_mx == mx and (n, nz, nb) == (len(lw_all), n_zero, n_bad)
    assert abs(got_s1 - s1) <= b * s1 and abs(got_s2 - s2) <= 2 * b * s2 and abs(got_sl - sl) <= b * sabs
    got = analysis.importance_summary(h)
    ess = s1 * s1 / s2 if s1 > 0 else 0.0
    assert abs(got["ess"] - ess) <= 4 * b * ess
    return got


def _rows(M, seed, spread=5.0):
    rng = np.random.default_rng(seed)
    return rng.normal(0, spread, M), rng.normal(-20, 3, M).astype(np.float32)


@pytest.mark.parametrize("M", [1, 63, 257, 1000])
def test_weights_kernel_matches_restatement(M):
    """One row, under one wave, two workgroups with a one-row tail, four workgroups."""
    beta = 0.8
    E, q = _rows(M, M)
    state = analysis.iw_state("cuda")
    lw = _weights(state, beta, E, q)
    want = -beta * _cuda(E) - _cuda(q).double()  # torch's own float64 expression
    assert torch.equal(lw, want)
    np.testing.assert_array_equal(lw.cpu().numpy(), log_weights(beta, E, q)[0])
    _check_header(analysis.iw_header(state), lw.cpu().numpy(), 0, 0)


def test_hard_core_and_nan_rows():
    """E = +inf rows weigh nothing (n_zero); a NaN log_q row is bad (n_bad) and never reaches
    a sum, whatever its energy; a -inf energy is bad too."""
    beta, M = 1.0, 300
    E, q = _rows(M, 3)
    E[[0, 17, 255, 256, 299]] = np.inf
    q[40] = np.nan
    q[41], E[41] = np.inf, np.inf  # bad wins over zero-weight
    E[42] = -np.inf
    E[43] = np.nan
    state = analysis.iw_state("cuda")
    lw = _weights(state, beta, E, q).cpu().numpy()
    want, zero, bad = log_weights(beta, E, q)
    np.testing.assert_array_equal(lw, want)
    assert zero.sum() == 5 and bad.sum() == 4 and not np.isnan(lw).any()
    fin = np.isfinite(lw)
    assert torch.equal(_cuda(lw[fin]), (-beta * _cuda(E) - _cuda(q).double())[_cuda(fin)])
    h = analysis.iw_header(state)
    assert not any(math.isnan(v) for v in h[:4])
    _check_header(h, lw, 5, 4)


def test_empty_weight_batch_then_recovery():
    """A batch of only -inf rows: max_lw = -inf, S1 = 0, ess = 0, no NaN; the weighted
    outputs of such a state are 0; a later finite batch recovers."""
    state = analysis.iw_state("cuda")
    lw0 = _weights(state, 1.0, np.full(70, np.inf), np.zeros(70, np.float32)).cpu().numpy()
    h = analysis.iw_header(state)
    assert h == (-np.inf, 0.0, 0.0, 0.0, 70, 70, 0) and (lw0 == -np.inf).all()
    assert analysis.importance_summary(h)["ess"] == 0.0
    out = _reduce_all(_configs(3, 70, 1), _half_box(3), _cuda(lw0), state, 10)
    assert not out["hist_w"].any() and not out["g_r_w"].any() and out["scalars"] == [0.0, 0.0, 0.0, 0.0]
    E, q = _rows(257, 9)
    lw1 = _weights(state, 1.0, E, q).cpu().numpy()
    _check_header(analysis.iw_header(state), np.concatenate([lw0, lw1]), 70, 0)


def test_spread_of_three_thousand():
    """Log-weights over +-1500: an unshifted exp would overflow and underflow."""
    M = 1000
    E = np.linspace(-1500.0, 1500.0, M)
    np.random.default_rng(0).shuffle(E)
    state = analysis.iw_state("cuda")
    lw = _weights(state, 1.0, E, np.zeros(M, np.float32)).cpu().numpy()
    assert lw.max() == 1500.0 and lw.min() == -1500.0
    got = _check_header(analysis.iw_header(state), lw, 0, 0)
    assert math.isfinite(got["log_z"]) and 1.0 <= got["ess"] < 3.0


def test_streaming_matches_one_batch_and_repeats_bitwise():
    """Three batches with the maximum in the second one against the same rows at once, both
    within the bound of the truth; the same call sequence twice gives the same bits."""
    beta = 1.3
    E, q = _rows(900, 21)
    E[450] = -60.0  # the largest log-weight by far, in the second batch
    cuts = [(0, 257), (257, 700), (700, 900)]

    def run(parts):
        state = analysis.iw_state("cuda")
        lw = torch.cat([_weights(state, beta, E[a:b], q[a:b]) for a, b in parts])
        return state[:8].clone(), lw

    s3, lw3 = run(cuts)
    s1, lw1 = run([(0, 900)])
    assert torch.equal(lw3, lw1) and int(lw1.argmax()) == 450
    lw = lw1.cpu().numpy()
    _check_header(analysis.iw_header(s3), lw, 0, 0)
    _check_header(analysis.iw_header(s1), lw, 0, 0)
    st = Stream()
    for a, b in cuts:
        st.add(beta, E[a:b], q[a:b])
    assert st.max_lw == analysis.iw_header(s3)[0] and abs(st.s1 - analysis.iw_header(s3)[1]) <= 2 * bound(lw) * st.s1
    again, _ = run(cuts)
    assert torch.equal(again, s3)


# ---------------------------------------------------------------- weighted analysis
def _configs(N, M, seed, hb=None):
    """Centred float32 samples in the box, with entries on the closed last edge and the first."""
    hb = _half_box(N) if hb is None else hb
    rng = np.random.default_rng(seed)
    z = np.clip(((rng.random((M, N, 2)) * 2 - 1) * hb).astype(np.float32), -np.float32(hb), np.float32(hb))
    z[0, 0] = (np.float32(hb), -np.float32(hb))
    return z


def _reduce_all(z, hb, lw, state, bins, r0=1.2):
    """fs_sample_analysis + fs_classify_wells on z, then the two weighted kernels with the
    given log-weights and finished state."""
    from test_gpu_a2_outputs import _launch

    M, N, _ = z.shape
    L, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
    samples, hist, counts, g = _launch(z, hb, bins=bins)
    _, denom, _ = analysis._rdf_bins(N, hb, hb / 50)
    cfg = _cuda(samples)
    _, well, avg_x = analysis.classify_wells(cfg, hb, r0)
    nb, nr = bins - 1, counts.shape[1]
    e2, d = _cuda(np.linspace(-hb, hb, bins)), _cuda(denom)
    g_w = torch.full((nr,), 9.0, dtype=torch.float64, device="cuda")
    sc = torch.full((4,), 9.0, dtype=torch.float64, device="cuda")
    hist_w = torch.zeros((nb, nb), dtype=torch.float64, device="cuda")
    _lib.check(L.fs_weighted_reduce(p(counts), M, nr, p(d), p(well), p(avg_x), p(lw), p(state), p(g_w), p(sc), st),
               "fs_weighted_reduce")
    _lib.check(L.fs_weighted_hist2d(p(cfg), M, N, hb, p(e2), nb, p(lw), p(state), p(hist_w), st), "fs_weighted_hist2d")
    torch.cuda.synchronize()
    return dict(samples=samples, hist=hist.cpu().numpy(), counts=counts.cpu().numpy(), g_r=g, denom=denom,
                well=well.cpu().numpy(), avg_x=avg_x.cpu().numpy(), g_r_w=g_w.cpu().numpy(), scalars=sc.tolist(),
                hist_w=hist_w.cpu().numpy(), edges=np.linspace(-hb, hb, bins))


def _close(got, want, b, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    print(f"{what}: max err / bound = {(err / np.maximum(b * np.abs(want), 1e-300)).max():.3e} (bound {b:.3e})")
    assert (err <= b * np.abs(want)).all(), what


def _check_weighted(out, lw):
    """The weighted outputs against fsum restatements with w~ from the truth."""
    w = normalised(lw)
    b = 2 * bound(lw)
    _close(out["hist_w"], weighted_hist(out["samples"], out["edges"][-1], out["edges"], w), b, "hist_w")
    ratio = out["counts"].astype(np.float64) / out["denom"]
    _close(out["g_r_w"], [math.fsum(w * ratio[:, k]) for k in range(ratio.shape[1])], b, "g_r_w")
    pa, pb = math.fsum(w[out["well"] == 1]), math.fsum(w[out["well"] == 2])
    _close(out["scalars"][0], pa, b, "p_a_w")
    _close(out["scalars"][1], pb, b, "p_b_w")
    _close(out["scalars"][3], math.fsum(w * out["avg_x"]), b, "avg_x_w")
    if pa > 0 and pb > 0:  # ln of a ratio of two sums, each within b: 2 b + the rounding of / and log
        assert abs(out["scalars"][2] - math.log(pb / pa)) <= 2 * b + 4 * U * max(1.0, abs(math.log(pb / pa)))
    else:
        assert out["scalars"][2] == 0.0


def _wells(z, hb, a_rows, b_rows, seed):
    """Put whole configurations inside well A (centred (-hb/2, 0)) and well B ((hb/2, 0))."""
    rng = np.random.default_rng(seed)
    N = z.shape[1]
    for rows, cx in ((a_rows, -hb / 2), (b_rows, hb / 2)):
        for m in rows:
            z[m] = (np.array([cx, 0.0]) + rng.uniform(-0.6, 0.6, (N, 2))).astype(np.float32)
    return z


def test_equal_weights_tie_to_the_unweighted_kernels():
    """lw constant over M = 128 rows: w~ = 2^-7 exactly, so 128 hist_w is
    fs_sample_analysis's integer hist, g_r_w is fs_rdf_mean's g_r, and p_a_w / p_b_w are
    fs_classify_wells' counts over 128."""
    N, M, hb = 3, 128, _half_box(3)
    z = _wells(_configs(N, M, 4), hb, range(10, 45), range(60, 81), 1)
    state = analysis.iw_state("cuda")
    lw = _weights(state, 1.0, np.full(M, 2.5), np.full(M, -7.25, np.float32))
    assert analysis.iw_header(state)[:2] == (4.75, 128.0)
    out = _reduce_all(z, hb, lw, state, 100)
    np.testing.assert_array_equal(out["hist_w"] * 128, out["hist"].astype(np.float64))
    _close(out["g_r_w"], out["g_r"], 2 * bound(lw.cpu().numpy()), "g_r_w against fs_rdf_mean")
    n_a, n_b = int((out["well"] == 1).sum()), int((out["well"] == 2).sum())
    assert n_a >= 35 and n_b >= 21
    assert out["scalars"][0] == n_a / 128 and out["scalars"][1] == n_b / 128
    assert abs(out["scalars"][2] - math.log(n_b / n_a)) <= 8 * U


@pytest.mark.parametrize("bins", [10, 100, 121])
@pytest.mark.parametrize("N", [3, 16])
def test_weighted_reductions_match_numpy(N, bins):
    """M = 130 is ragged against four waves per workgroup; bins = 121 is the LDS maximum
    (120 x 120 float64 bins); hard-core rows are skipped."""
    M, hb = 130, _half_box(N)
    z = _configs(N, M, 10 * N + bins)
    if N == 3:
        z = _wells(z, hb, range(5, 40), range(70, 100), 2)
    E, q = _rows(M, bins + N, spread=3.0)
    E[[7, 129]] = np.inf
    state = analysis.iw_state("cuda")
    lw = _weights(state, 1.0, E, q)
    out = _reduce_all(z, hb, lw, state, bins)
    _check_weighted(out, lw.cpu().numpy())
    if N == 3:
        assert out["scalars"][0] > 0 and out["scalars"][1] > 0


def test_one_configuration_carries_all_the_weight():
    """Every other weight underflows to 0 against the maximum: the outputs are that
    configuration's own counts, exactly."""
    N, M, hb = 16, 130, _half_box(16)
    z = _configs(N, M, 77)
    E = np.full(M, 2000.0)
    E[97] = 0.0
    state = analysis.iw_state("cuda")
    lw = _weights(state, 1.0, E, np.zeros(M, np.float32))
    assert analysis.iw_header(state)[:3] == (0.0, 1.0, 1.0)
    out = _reduce_all(z, hb, lw, state, 100)
    own = weighted_hist(out["samples"][97:98], hb, out["edges"], np.ones(1))
    np.testing.assert_array_equal(out["hist_w"], own)
    np.testing.assert_array_equal(out["g_r_w"], out["counts"][97] / out["denom"])
    assert out["scalars"][3] == out["avg_x"][97]


def test_all_particles_in_one_bin():
    """The heaviest contention on one LDS bin and one global bin."""
    N, M, hb = 16, 130, _half_box(16)
    edges = np.linspace(-hb, hb, 100)
    lo, wd = edges[60], edges[61] - edges[60]
    rng = np.random.default_rng(3)
    z = (lo + wd * (0.25 + 0.5 * rng.random((M, N, 2)))).astype(np.float32)
    E, q = _rows(M, 31, spread=2.0)
    state = analysis.iw_state("cuda")
    lw = _weights(state, 1.0, E, q)
    out = _reduce_all(z, hb, lw, state, 100)
    assert np.count_nonzero(out["hist_w"]) == 1
    _close(out["hist_w"][60, 60], float(N), 2 * bound(lw.cpu().numpy()), "the one bin")
    _check_weighted(out, lw.cpu().numpy())


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def flow_run():
    """sample_analysis on the Algorithm-2 test flow (N = 3, 1500 samples asked, two batches
    of 1000 kept) three ways from the same generator seed."""
    from test_gpu_algorithm2 import _cycle_model

    m = _cycle_model().cuda().eval()
    B = float(m.flows[0].tail_bound)
    phys = Physics(2 * B)

    def run(**kw):
        g = torch.Generator(device="cuda")
        g.manual_seed(123)
        return analysis.sample_analysis(m, 1500, B, generator=g, **kw)

    return m, phys, run(), run(reweight=phys), run(reweight=phys, density_pass=True)


def test_reweighting_leaves_the_existing_keys_bit_identical(flow_run):
    _, _, plain, single, dens = flow_run
    assert set(plain) == {"samples", "hist", "x_edges", "y_edges", "r_vals", "g_r"}
    for res in (single, dens):
        assert torch.equal(res["samples"], plain["samples"]) and torch.equal(res["hist"], plain["hist"])
        for k in ("g_r", "x_edges", "y_edges", "r_vals"):
            np.testing.assert_array_equal(res[k], plain[k])


def test_sample_analysis_weights_end_to_end(flow_run):
    m, phys, _, single, dens = flow_run
    samples = single["samples"]
    assert samples.shape == (2000, 3, 2)
    E, W, _ = total_energy(samples, phys.c)
    assert torch.equal(single["energy"], E) and torch.equal(dens["energy"], E)
    for res in (single, dens):
        assert res["log_q"].dtype == torch.float32 and res["log_w"].dtype == torch.float64
        assert torch.equal(res["log_w"], -phys.beta * res["energy"] - res["log_q"].double())
    init = samples[:4].double().cpu().numpy()
    bmc = BatchedMonteCarlo(m, init, phys, [1, 2, 3, 4], device="cuda")
    E2, _, lq2 = bmc.proposal_terms(samples)
    bmc.check_errors()
    assert torch.equal(dens["log_q"], lq2) and torch.equal(dens["energy"], E2)
    # the sampling pass's own log q against the density pass: tests/test_gpu_mh.py's tolerance
    rel = ((single["log_q"].double() - lq2.double()).abs() / lq2.double().abs()).cpu().numpy()
    assert np.median(rel) < 1e-5 and rel.max() < 1e-3, (np.median(rel), rel.max())
    for res in (single, dens):
        lw = res["log_w"].cpu().numpy()
        mx, s1, s2, sl, sabs = truth(lw)
        b = bound(lw)
        n_zero = int((lw == -np.inf).sum())
        assert (res["n_zero"], res["n_bad"]) == (n_zero, 0)
        ess = s1 * s1 / s2
        assert abs(res["ess"] - ess) <= 4 * b * ess and res["ess_fraction"] == res["ess"] / 2000
        # log Z = max + log(S1 / n): S1 within b, then the rounding of /, log and +
        lz = mx + math.log(s1 / 2000)
        assert abs(res["log_z"] - lz) <= b + 4 * U * max(1.0, abs(lz), abs(mx))
        assert abs(res["mean_log_w"] - sl / (2000 - n_zero)) <= (b * sabs + 2 * U * abs(sl)) / (2000 - n_zero)
        assert abs(res["max_weight_fraction"] - 1 / s1) <= 2 * b / s1
        assert 1.0 <= res["ess"] <= 2000 and 0 < res["max_weight_fraction"] <= 1
        out = dict(samples=samples.cpu().numpy(), edges=res["x_edges"], hist_w=res["hist_w"], g_r_w=res["g_r_w"],
                   scalars=[res["p_a_w"], res["p_b_w"], res["deltaF_w"], res["avg_x_w"]])
        _, well, avg_x = analysis.classify_wells(samples, phys.half_width, 1.2)
        r_edges, denom, _ = analysis._rdf_bins(3, phys.half_width, phys.half_width / 50)
        out.update(well=well.cpu().numpy(), avg_x=avg_x.cpu().numpy(), denom=denom,
                   counts=analysis.pair_histograms(samples - np.float32(phys.half_width), phys.half_width,
                                                   r_edges).cpu().numpy())
        _check_weighted(out, lw)
        assert res["p_a"] == (out["well"] == 1).sum() / 2000 and res["p_b"] == (out["well"] == 2).sum() / 2000
        assert abs(res["hist_w"].sum() - 3.0) <= 3.0 * 2 * b + 3.0 * 8 * U  # every particle is in the box


def test_reweight_needs_the_same_box(flow_run):
    m = flow_run[0]
    B = float(m.flows[0].tail_bound)
    with pytest.raises(ValueError, match="box"):
        analysis.sample_analysis(m, 10, B, batch=10, reweight=Physics(2 * B + 1))


# ---------------------------------------------------------------- Algorithm 2
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    from test_gpu_a2_outputs import _driver

    kw = dict(checkpoint_interval=2, num_samples_for_analysis=1500, initial_p_acc=0.0,
              initial_training_num_samples=5000, cmap_name="ICL_diverging")
    d0, d1 = str(tmp_path_factory.mktemp("plain")), str(tmp_path_factory.mktemp("reweighted"))
    return _driver(out_dir=d0, **kw) + (d0,), _driver(out_dir=d1, reweight_analysis=True, **kw) + (d1,)


def test_run_writes_the_importance_files(drivers):
    (_, a0, _, _, d0), (_, a1, _, _, d1) = drivers
    assert not [f for f in os.listdir(d0) if f.startswith("importance")]
    assert sorted(f for f in os.listdir(d1) if f.startswith("importance")) == \
        ["importance_cycle_2_data.json", "importance_cycle_3_data.json"]
    assert "log_w" not in a0.last_analysis
    res = a1.last_analysis
    data = json.load(open(os.path.join(d1, "importance_cycle_3_data.json")))
    from flowstate.io import IMPORTANCE_SCALARS
    for k in IMPORTANCE_SCALARS:
        assert data[k] == res[k], k
    assert data["n_zero"] + data["n_bad"] < 2000 and 1.0 <= data["ess"] <= 2000
    np.testing.assert_array_equal(np.array(data["g_r_w"]), res["g_r_w"])
    np.testing.assert_array_equal(np.array(data["hist_w"]), res["hist_w"])
    np.testing.assert_array_equal(np.array(data["r"]), res["r_vals"])
    assert np.array(data["hist_w"]).shape == (99, 99)


def test_reweighted_run_leaves_chains_and_files_unchanged(drivers):
    from test_gpu_a2_outputs import CHAIN_STATE

    (b0, a0, o0, _, d0), (b1, a1, o1, _, d1) = drivers
    for (s0, l0, c0, p0), (s1, l1, c1, p1) in zip(o0, o1):
        assert torch.equal(s0.xy, s1.xy) and l0 == l1 and p0 == p1 and torch.equal(c0, c1)
    for k in CHAIN_STATE:
        assert torch.equal(getattr(b0, k), getattr(b1, k)), k
    old = sorted(os.listdir(d0))
    assert old == sorted(f for f in os.listdir(d1) if not f.startswith("importance")) and len(old) >= 8
    for f in old:
        p0, p1 = os.path.join(d0, f), os.path.join(d1, f)
        if f.endswith(".json"):
            j0, j1 = json.load(open(p0)), json.load(open(p1))
            j0.pop("directory", None), j1.pop("directory", None)  # the output directory's own name
            assert j0 == j1, f
        elif f.endswith(".pth"):
            w0, w1 = torch.load(p0), torch.load(p1)
            assert w0.keys() == w1.keys() and all(torch.equal(w0[k], w1[k]) for k in w0), f
        else:
            assert open(p0, "rb").read() == open(p1, "rb").read(), f
