"""Algorithm-2 checkpoint-cycle analysis on the GPU: fs_sample_analysis (one launch per
analysis batch: samples + HALF_BOX, the heat-map counts and the pair-distance counts of
samples - HALF_BOX, all float32) with fs_rdf_mean against the reference's own outputs
(tests/golden/a2_outputs.npz) and against their numpy restatement
(test_a2_outputs_cpu.restate, pinned to the same fixture) at the shapes where the kernel
takes other paths; then Algorithm2.run with checkpoint_interval: the files of
main_algorithm_2.py:458-526 / 588-599, and chains identical to a run without
checkpoints.  Every comparison is exact."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from flowstate import _lib, analysis
from flowstate.algorithm2 import Algorithm2
from flowstate.MCMC import BatchedMonteCarlo, Physics, initialise_low_left, initialise_low_right
from test_a2_outputs_cpu import CASES, analyse, restate

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHAIN_STATE = ("state", "state_is_f32", "pcg", "pcg_buf", "max_disp", "attempts", "accepted", "E_old", "W_old",
               "nll_old", "n_accept")


def _half_box(N):
    return ((N / 0.03) ** (1 / 2)) / 2


def _launch(z, hb, bins=100, dr=None, hist=None, counts=None, row0=0):
    """fs_sample_analysis on z (numpy float32 (M, N, 2)) into rows row0.. of counts, then
    fs_rdf_mean over all rows of counts -> samples, hist, counts, g_r (numpy) and the
    device hist / counts for a following call."""
    M, N, _ = z.shape
    dr = hb / 50 if dr is None else dr
    r_edges, denom, _ = analysis._rdf_bins(N, hb, dr)
    e2 = torch.from_numpy(np.linspace(-hb, hb, bins)).cuda()
    er = torch.from_numpy(r_edges).cuda()
    nb, nr = bins - 1, r_edges.shape[0] - 1
    if hist is None:
        hist = torch.zeros((nb, nb), dtype=torch.int64, device="cuda")
    if counts is None:
        counts = torch.full((M, nr), -7, dtype=torch.int32, device="cuda")
    out = torch.full((M, N, 2), float("nan"), dtype=torch.float32, device="cuda")
    analysis.sample_analysis_batch(torch.from_numpy(z).cuda(), hb, e2, er, out, hist, counts[row0:row0 + M])
    g = torch.empty(nr, dtype=torch.float64, device="cuda")
    done = row0 + M
    _lib.check(_lib.load().fs_rdf_mean(_lib.ptr(counts), done, nr, _lib.ptr(torch.from_numpy(denom).cuda()),
                                       _lib.ptr(g), _lib.stream_ptr()), "fs_rdf_mean")
    torch.cuda.synchronize()
    return out.cpu().numpy(), hist, counts, g.cpu().numpy()


def _inputs(N, M, seed, hb):
    rng = np.random.default_rng(seed)
    z = ((rng.random((M, N, 2)) * 2 - 1) * hb).astype(np.float32)
    return np.clip(z, -np.float32(hb), np.float32(hb))


@pytest.mark.parametrize("name", CASES)
def test_kernel_reproduces_reference_outputs(name):
    f = np.load(os.path.join(G, "a2_outputs.npz"))
    hb = float(f[name + "/half_box"])
    samples, hist, _, g = _launch(f[name + "/z"], hb)
    np.testing.assert_array_equal(samples, f[name + "/samples"])
    h = hist.cpu().numpy().astype(np.float64)
    np.testing.assert_array_equal(h / h.sum(), f[name + "/hist_relative"])
    np.testing.assert_array_equal(g, f[name + "/g_r"])


@pytest.mark.parametrize("bins", [100, 121])
@pytest.mark.parametrize("N,M", [(3, 5), (64, 130), (65, 9), (256, 4)])
def test_kernel_matches_restatement(N, M, bins):
    """One wave per configuration and four per workgroup: M below, above and off the
    multiples of 4; N below, at and above one lane loop (64), and the largest (256);
    nb = 99 (the driver's) and 120 (the LDS bound)."""
    hb = _half_box(N)
    z = _inputs(N, M, 100 + N, hb)
    z[0, 0] = (np.float32(hb), -np.float32(hb))  # the closed last edge and the first edge
    z[M - 1, N - 1] = z[M - 1, 0]  # a zero distance in the last row
    samples, hist, counts, g = _launch(z, hb, bins=bins)
    a_, want_hist, _, _, want_g = restate(z, hb, bins=bins)
    np.testing.assert_array_equal(samples, a_)
    np.testing.assert_array_equal(hist.cpu().numpy(), want_hist.astype(np.int64))
    # (a particle at +-fl32(hb) is outside the float64 edges when fl32(hb) rounds up, as in numpy)
    assert M * N - 2 <= int(hist.sum()) <= M * N and bool((counts >= 0).all())
    np.testing.assert_array_equal(g, want_g)


def test_kernel_at_the_largest_histograms():
    """nb = 120 with nr = 128: the largest LDS request (past 64 KiB, dynamic)."""
    hb = _half_box(3)
    z = _inputs(3, 5, 7, hb)
    samples, hist, _, g = _launch(z, hb, bins=121, dr=hb / 128)
    a_, want_hist, _, r, want_g = restate(z, hb, bins=121, dr=hb / 128)
    assert g.shape == (128,) and r.shape == (128,)
    np.testing.assert_array_equal(samples, a_)
    np.testing.assert_array_equal(hist.cpu().numpy(), want_hist.astype(np.int64))
    np.testing.assert_array_equal(g, want_g)


def test_all_particles_in_one_bin():
    """Every particle of the batch in one heat-map bin (the heaviest contention on one
    LDS counter and one global bin)."""
    N, M = 64, 130
    hb = _half_box(N)
    edges = np.linspace(-hb, hb, 100)
    lo, w = edges[60], edges[61] - edges[60]
    rng = np.random.default_rng(3)
    z = (lo + w * (0.1 + 0.8 * rng.random((M, N, 2)))).astype(np.float32)
    samples, hist, _, g = _launch(z, hb)
    a_, want_hist, _, _, want_g = restate(z, hb)
    assert np.count_nonzero(want_hist) == 1 and want_hist[60, 60] == M * N
    np.testing.assert_array_equal(samples, a_)
    np.testing.assert_array_equal(hist.cpu().numpy(), want_hist.astype(np.int64))
    np.testing.assert_array_equal(g, want_g)


def test_successive_batches_accumulate():
    """Two batches of one checkpoint: hist accumulates, counts rows land at the batch's
    offset, rows outside the batch stay as they were, g(r) is over all rows."""
    N, M = 16, 9
    hb = _half_box(N)
    z0, z1 = _inputs(N, M, 11, hb), _inputs(N, M, 12, hb)
    counts = torch.full((2 * M, 50), -7, dtype=torch.int32, device="cuda")
    _, hist, counts, _ = _launch(z0, hb, counts=counts, row0=0)
    assert bool((counts[M:] == -7).all()) and bool((counts[:M] >= 0).all())
    first = counts[:M].clone()
    h0 = restate(z0, hb)[1]
    np.testing.assert_array_equal(hist.cpu().numpy(), h0.astype(np.int64))
    _, hist, counts, g = _launch(z1, hb, hist=hist, counts=counts, row0=M)
    assert torch.equal(counts[:M], first)
    _, h01, _, _, want_g = restate(np.concatenate([z0, z1]), hb)
    np.testing.assert_array_equal(hist.cpu().numpy(), h01.astype(np.int64))
    np.testing.assert_array_equal(g, want_g)


@pytest.mark.parametrize("N,nb,nr", [(16, 121, 50), (16, 99, 129), (257, 99, 50)])
def test_out_of_range_sizes_launch_nothing(N, nb, nr):
    M = 4
    z = torch.zeros((M, N, 2), dtype=torch.float32, device="cuda")
    e2 = torch.linspace(-1, 1, nb + 1, dtype=torch.float64, device="cuda")
    er = torch.linspace(0, 1, nr + 1, dtype=torch.float64, device="cuda")
    out = torch.full_like(z, 3.0)
    hist = torch.full((nb, nb), 5, dtype=torch.int64, device="cuda")
    counts = torch.full((M, nr), -7, dtype=torch.int32, device="cuda")
    L = _lib.load()
    rc = L.fs_sample_analysis(_lib.ptr(z), M, N, 1.0, _lib.ptr(e2), nb, _lib.ptr(er), nr, _lib.ptr(out),
                              _lib.ptr(hist), _lib.ptr(counts), _lib.stream_ptr())
    assert rc == -1 and b"fs_sample_analysis" in L.fs_last_error()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((hist == 5).all()) and bool((counts == -7).all())
    assert L.fs_sample_analysis(None, 0, 16, 1.0, _lib.ptr(e2), 99, _lib.ptr(er), 50, None, None, None,
                                ctypes.c_void_p(0)) == 0  # M = 0 with sizes in range: success, nothing to do


# ---------------------------------------------------------------- driver
def _driver(**kw):
    from test_gpu_algorithm2 import _cycle_model

    N, runs = 3, 100
    m = _cycle_model()
    B = float(m.flows[0].tail_bound)
    init = np.array([(initialise_low_left if i % 2 == 0 else initialise_low_right)(N, 0.03, 1.0)[0]
                     for i in range(runs)])
    bmc = BatchedMonteCarlo(None, init, Physics(2 * B), [42 + i for i in range(runs)], device="cuda",
                            initial_max_displacement=0.65)
    bmc.local_moves(500, adjust_every=100)
    a = Algorithm2(bmc, m, batch_size=256, alpha=1.0, sampling_frequency=10, update_num_samples=1000, **kw)
    torch.manual_seed(0)
    out = a.run(3)
    torch.cuda.synchronize()
    return bmc, a, out, B


@pytest.fixture(scope="module")
def checkpointed(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("a2"))
    return _driver(checkpoint_interval=2, num_samples_for_analysis=1500, out_dir=d, initial_p_acc=0.0,
                   initial_training_num_samples=5000, cmap_name="ICL_diverging") + (d,)


def test_run_writes_the_checkpoint_files(checkpointed):
    bmc, a, out, hb, d = checkpointed
    s = np.load(os.path.join(d, "samples.npy"))
    assert s.dtype == np.float32 and s.shape == (2000, 3, 2)
    assert s.min() >= 0 and s.max() <= 2 * np.float32(hb)
    for c in (1, 2, 3):
        for name in (f"frequency_heatmap_cycle_{c}_data.json", f"pair_correlation_function_{c}_data.json",
                     f"model_checkpoint_cycle_{c}.pth"):
            assert os.path.exists(os.path.join(d, name)) == (c != 1), name
    hist, edges, r, g = analyse(s, hb)
    hm = json.load(open(os.path.join(d, "frequency_heatmap_cycle_3_data.json")))
    np.testing.assert_array_equal(np.array(hm["hist_relative"]), hist / hist.sum())
    np.testing.assert_array_equal(np.array(hm["x_edges"]), edges)
    np.testing.assert_array_equal(np.array(hm["y_edges"]), edges)
    assert hm["cmap_name"] == "ICL_diverging"
    pc = json.load(open(os.path.join(d, "pair_correlation_function_3_data.json")))
    np.testing.assert_array_equal(np.array(pc["r"]), r)
    np.testing.assert_array_equal(np.array(pc["g_r"]), g)
    from test_gpu_algorithm2 import _cycle_model

    live = a.model.state_dict()
    for c in (2, 3):
        sd = torch.load(os.path.join(d, f"model_checkpoint_cycle_{c}.pth"), weights_only=True)
        _cycle_model().load_state_dict(sd, strict=True)
        same = all(torch.equal(sd[k].cpu(), live[k].cpu()) for k in live)
        assert same == (c == 3)
    pa = json.load(open(os.path.join(d, "p_acc_history_data.json")))
    assert pa["total_samples_trained"] == [5000, 6000, 7000, 8000]
    assert pa["p_acc_history"] == [0.0] + [p for _, _, _, p in out]
    assert json.load(open(os.path.join(d, "loss_function_data.json")))["loss_epoch"] == [l for _, l, _, _ in out]
    (avg_x, p_a, p_b, dF), curve = a.well_statistics([o[0] for o in out], 5)
    assert avg_x.shape == p_a.shape == p_b.shape == dF.shape == (100, 25) and curve[0].shape == (25,)


def test_checkpoints_do_not_disturb_the_chains(checkpointed):
    """The analysis batch draws from a generator of its own on the main stream: accepts,
    p_acc, losses and the final runs are bit-identical to a run without checkpoints."""
    b1, a1, o1, _, _ = checkpointed
    b0, a0, o0, _ = _driver()
    assert a0.checkpoint_interval is None and a0.last_analysis is None and a1.last_analysis is not None
    for (s0, l0, c0, p0), (s1, l1, c1, p1) in zip(o0, o1):
        assert torch.equal(s0.xy, s1.xy) and l0 == l1 and p0 == p1 and torch.equal(c0, c1)
    assert a0.p_acc_history == a1.p_acc_history
    for k in CHAIN_STATE:
        assert torch.equal(getattr(b0, k), getattr(b1, k)), k
