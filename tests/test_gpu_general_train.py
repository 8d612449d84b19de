"""Training in the general-shape mode ("f32-general") at bin counts no coupling kernel is
instantiated for: the runtime-K coupling kernels (fs_coupling.any_k,
csrc/spline_autograd.hip) behind density_step / sample_step, the shared-launch step
(paired_kld), GraphedTrainStep and Algorithm2.  Each test repeats one of
tests/test_gpu_train_fused.py, test_gpu_paired.py, test_gpu_general.py or
test_gpu_algorithm2.py with that test's bounds, at the smallest shapes that reach the code
path: ragged row counts, D = 2, K = 1, K = 31, n = 64 (every lane of a wave on)."""
import copy

import numpy as np
import pytest
import torch

from flowstate import _lib
from flowstate.algorithm2 import Algorithm2
from flowstate.MCMC import BatchedMonteCarlo, Physics
from flowstate.models import build_flow, flow_from_state_dict, half_box
from flowstate.normflows import autograd_flow as AF
from flowstate.normflows.Energy import DoubleWellLJ
from flowstate.normflows.train import GraphedTrainStep, step_loss
from oracle import flow as OF
from oracle import physics as OP
from test_gpu_flow import close as oracle_close
from test_gpu_paired import _batch, _state, coupling_waves, no_fold  # noqa: F401 (no_fold: a fixture)
from test_gpu_train_fused import close

pytestmark = pytest.mark.gpu

MODE = "f32-general"


def _model(N, kw, seed=0, mode=MODE):
    """test_gpu_paired._model in the given precision mode."""
    torch.manual_seed(seed)
    B = half_box(N)
    m = build_flow(N, bound=B, device="cpu", **kw)
    m.p = DoubleWellLJ(2 * N, N, 1.0, B, V0_list=[-10.0, -10.5], r0=1.2, k=15)
    m = m.cuda().train().set_precision(mode)
    m.q0.device = torch.device("cuda")
    return m


def general_layer(seed, N, H, K):
    """test_gpu_train_fused.a2_layer in the general mode."""
    torch.manual_seed(seed)
    m = build_flow(N, bound=half_box(N), device="cpu", L=1, H=H, nb=2, K=K).set_precision(MODE)
    layer = m.flows[0]
    with torch.no_grad():  # leave the identity init: non-trivial splines and BatchNorm
        for prm in layer.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    return layer.cuda()


def _buffers_close(layer, ref):
    for (n, b1), (_, b2) in zip(layer.named_buffers(), ref.named_buffers()):
        if b1.dtype == torch.int64:
            assert torch.equal(b1, b2), n
        else:
            close(b1, b2, 1e-5, n)


LAYER_SHAPES = [(1, 24, 1), (3, 24, 7), (15, 96, 16), (64, 100, 20), (64, 128, 31)]  # (N, H, K)
ROWS = 70  # no multiple of anything the kernels tile by


# --- 1. a single layer against torch ops ---------------------------------------------
@pytest.mark.parametrize("N,H,K", LAYER_SHAPES, ids=str)
def test_density_step_matches_torch_ops_at_any_k(N, H, K):
    """test_density_step_matches_torch_ops on the runtime-K kernels
    (fs_coupling_features_* + fs_coupling_density_* with any_k) against coupling_density
    over torch ops and the element-wise runtime-K spline."""
    layer = general_layer(5, N, H, K)
    ref = copy.deepcopy(layer)
    layer.train()
    ref.train()
    B = layer.tail_bound
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.rand(ROWS, layer.num_input_channels, device="cuda", generator=g) * 2 - 1) * B
    x[:8, :5] = B * 1.5  # outside the tails: identity, log-det 0
    x[9:12, -1] = -B * 1.2
    lq0 = torch.randn(ROWS, device="cuda", generator=g)
    x1 = x.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    assert AF.fused_coupling_ok(layer, x1)
    assert AF._coupling_desc(layer, ROWS).any_k == 1
    z1, lq1 = AF.density_step(layer, x1, lq0)
    z2, ld2 = AF.coupling_density(ref, x2)
    lq2 = lq0 + ld2
    close(z1, z2, 1e-5, "z")
    close(lq1, lq2, 1e-5, "log q")
    gz = torch.randn_like(z1)
    gl = torch.randn_like(lq1)
    ((z1 * gz).sum() + (lq1 * gl).sum()).backward()
    ((z2 * gz).sum() + (lq2 * gl).sum()).backward()
    AF.check_nan_flags()
    close(x1.grad, x2.grad, 1e-4, "x grad")
    for (n, p1), (_, p2) in zip(layer.named_parameters(), ref.named_parameters()):
        if p2.grad is None:
            assert p1.grad is None or not p1.grad.abs().max().item(), n
            continue
        close(p1.grad, p2.grad, 1e-4, n)
    _buffers_close(layer, ref)


@pytest.mark.parametrize("N,H,K", LAYER_SHAPES, ids=str)
def test_sample_step_matches_torch_ops_at_any_k(N, H, K):
    """test_sample_step_matches_torch_ops on fs_coupling_sample_pre / _post with any_k."""
    layer = general_layer(6, N, H, K)
    ref = copy.deepcopy(layer)
    layer.train()
    ref.train()
    B = layer.tail_bound
    g = torch.Generator(device="cuda").manual_seed(2)
    z = (torch.rand(ROWS, layer.num_input_channels, device="cuda", generator=g) * 2 - 1) * B
    z[3:6, :2] = -B * 1.2
    z[20:22, -1] = B * 1.5
    lq0 = torch.randn(ROWS, device="cuda", generator=g)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert AF.fused_coupling_ok(layer, z)
    with torch.no_grad():
        z1, lq1 = AF.sample_step(layer, z, lq0, flag)
        z2, ld2 = AF.coupling_sample(ref, z)
        AF._nan_flags.clear()
    close(z1, z2, 1e-5, "z")
    close(lq1, lq0 - ld2, 1e-5, "log q")
    assert int(flag.item()) == 0
    _buffers_close(layer, ref)


# --- 2. runtime-K against instantiated kernels ----------------------------------------
@pytest.fixture
def force_any_k():
    prev = AF._force_any_k

    def set_(on):
        AF._force_any_k = on

    yield set_
    AF._force_any_k = prev


@pytest.mark.parametrize("K", [5, 8, 15, 32])
@pytest.mark.parametrize("N,kw,rows", [(16, dict(L=3, H=32, nb=1), 37), (64, dict(L=2, H=128, nb=2), 64)],
                         ids=["n16-ragged", "n64-h128"])
def test_runtime_k_kernels_match_instantiated(N, kw, rows, K, force_any_k):
    """The paired step in the default mode with every coupling launch forced onto the
    runtime-K kernels (AF._force_any_k) against the instantiated kernels: the same operations
    in the same order, so the loss agrees within float32 rounding of its sum, the gradients
    within the reassociation bound of test_bn_fold_matches_unfolded, the running statistics
    within 1e-5."""
    kw = dict(kw, K=K)
    outs = []
    for force in (False, True):
        force_any_k(force)
        m = _model(N, kw, seed=2, mode="f32")
        fbn = AF.FlatBatchNorm(m)
        x = _batch(N, rows, seed=6)
        x[::7, ::5] *= 1.2  # beyond the bound: the identity branches
        assert AF._coupling_desc(m.flows[0], rows).any_k == int(force)
        for p in m.parameters():
            p.grad = None
        torch.cuda.manual_seed(13)
        z = m.q0(rows).cuda()
        assert AF.paired_ok(m, x, z, fbn)
        torch.cuda.manual_seed(13)
        loss = step_loss(m, x, rows, 1.0, fbn)
        loss.backward()
        torch.cuda.synchronize()
        outs.append((loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None},
                     {n: b.clone() for n, b in m.named_buffers()}))
    (la, ga, ba), (lb, gb, bb) = outs
    torch.testing.assert_close(lb, la, rtol=2e-6, atol=0)
    assert ga.keys() == gb.keys()
    for n in ga:
        scale = float(ga[n].abs().max()) + 1e-30
        torch.testing.assert_close(gb[n], ga[n], rtol=1e-4, atol=2e-5 * scale, msg=n)
    for n in ba:
        if ba[n].is_floating_point():
            close(bb[n], ba[n], 1e-5, n)
        else:
            assert torch.equal(ba[n], bb[n]), n


# --- 3. the paired step equals the separate passes ------------------------------------
GENERAL_PAIRED = [(16, dict(L=4, H=64, nb=2, K=10), 96), (3, dict(L=3, H=40, nb=1, K=7), 37)]


@pytest.mark.parametrize("N,kw,rows", GENERAL_PAIRED, ids=["n16-k10", "n3-k7-ragged"])
def test_paired_step_matches_separate_passes_at_any_k(N, kw, rows, no_fold):
    """test_paired_step_matches_separate_passes at uninstantiated bin counts."""
    ma, mb = _model(N, kw), _model(N, kw)
    fbn = AF.FlatBatchNorm(mb)
    x = _batch(N, rows)
    z = mb.q0(rows).cuda()
    assert AF.paired_ok(mb, x, z, fbn)
    for m in (ma, mb):
        for p in m.parameters():
            p.grad = None
    torch.cuda.manual_seed(11)
    la = step_loss(ma, x, rows, 1.0)
    la.backward()
    torch.cuda.manual_seed(11)
    lb = step_loss(mb, x, rows, 1.0, fbn)
    lb.backward()
    torch.cuda.synchronize()
    torch.testing.assert_close(la, lb, rtol=2e-6, atol=0)
    for (na, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert (pa.grad is None) == (pb.grad is None), na
        if pa.grad is not None:
            assert torch.equal(pa.grad, pb.grad), na
    for (na, ba), (_, bb) in zip(ma.named_buffers(), mb.named_buffers()):
        assert torch.equal(ba, bb), na
    assert int(fbn.nbt[0]) == 2


# --- 4. launch count -------------------------------------------------------------------
def test_paired_launch_count_at_any_k():
    """test_paired_launch_count at K = 10: 7 launches per layer (+ 1) carry both passes,
    16 per layer when they run one after the other."""
    from torch.profiler import ProfilerActivity, profile

    N, rows = 16, 64
    kw = dict(L=4, H=64, nb=2, K=10)
    m = _model(N, kw)
    fbn = AF.FlatBatchNorm(m)
    x = _batch(N, rows)
    counts = {}
    for mode in ("paired", "separate"):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            loss = step_loss(m, x, rows, 1.0, fbn if mode == "paired" else None)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        if not names:
            pytest.skip("the profiler recorded no device kernels")
        counts[mode] = sum(1 for n in names if "gemm" in n or "coupling" in n)
        del loss
    L = kw["L"]
    assert counts["paired"] == 7 * L + 1, counts
    assert counts["separate"] == 16 * L, counts


# --- 5. wave variants ------------------------------------------------------------------
@pytest.mark.parametrize("N,kw,rows", [(16, dict(L=3, H=32, nb=1, K=10), 37), (8, dict(L=3, H=32, nb=1, K=31), 50),
                                       (64, dict(L=2, H=64, nb=1, K=10), 40)],
                         ids=["n16-k10", "n8-k31", "n64-k10"])
def test_coupling_waves_bit_identical_at_any_k(N, kw, rows):
    """test_coupling_waves_bit_identical on the runtime-K kernels."""
    outs = []
    for on in (1, 0):
        with coupling_waves(on):
            m = _model(N, kw, seed=2)
            fbn = AF.FlatBatchNorm(m)
            x = _batch(N, rows, seed=6)
            x[::7, ::5] *= 1.2  # beyond the bound: the identity branches
            for p in m.parameters():
                p.grad = None
            torch.cuda.manual_seed(13)
            z = m.q0(rows).cuda()
            assert AF.paired_ok(m, x, z, fbn)
            torch.cuda.manual_seed(13)
            loss = step_loss(m, x, rows, 1.0, fbn)
            loss.backward()
            torch.cuda.synchronize()
            outs.append([loss.detach().clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None]
                        + [b.clone() for b in m.buffers()])
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# --- 6. graphed steps ------------------------------------------------------------------
def test_paired_graphed_steps_match_separate_at_any_k(no_fold):
    """test_paired_graphed_steps_match_separate at K = 10 in the general mode."""
    N, rows = 16, 128
    kw = dict(L=4, H=64, nb=2, K=10)
    out = []
    for paired in (True, False):
        m = _model(N, kw, seed=4)
        x = _batch(N, rows, seed=5)
        torch.cuda.manual_seed(7)
        g = GraphedTrainStep(m, rows, lr=1e-3, weight_decay=1e-4, alpha=1.0, example=x, paired=paired)
        assert (g.flat_bn is not None) == paired
        for k in range(3):
            g.step(_batch(N, rows, seed=10 + k))
        torch.cuda.synchronize()
        out.append(_state(m) + [t.clone() for t in g._state_tensors])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_graphed_step_matches_cpu_module():
    """One graphed step at (N, L, H, nb, K) = (3, 2, 40, 1, 7), batch 64, against the same
    module stepped on the CPU (torch restatement, torch's Adam), with the bounds of
    test_training_step_in_general_mode: loss rtol 2e-5; gradients rtol 2e-3, atol 2e-5.

    The parameters: Adam's first step moves an element by -lr g / (|g| + eps), so the
    gradient bound carries over to the parameters (scaled by lr: rtol 2e-3 of the move,
    atol 2e-5 lr) wherever it fixes the gradient's sign and keeps |g| far above eps; that
    is |g| > 1e-3, 50 times the gradient's atol.  A smaller gradient may change sign within
    its bound, and then the two moves differ by up to 2 lr: there the test asks for that.
    Then the general-mode log_prob on the new weights against the oracle on the same."""
    shape = (3, 2, 40, 1, 7)
    N, L, H, nb, K = shape
    lr, rows = 1e-2, 64
    dims = OF.FlowDims(N=N, L=L, H=H, nb=nb, K=K, B=half_box(N))
    sd = OF.random_state_dict(dims, seed=7, final_std=0.05)
    g = torch.Generator().manual_seed(2)
    x = (torch.rand((rows, dims.D), generator=g) * 2 - 1) * dims.B
    # the CPU module: forward_kld is the step's loss at ALPHA = 1 (the reverse term's weight is 0)
    mc = build_flow(N, L, H, nb, K, bound=dims.B, device="cpu")
    mc.load_state_dict(sd, strict=True)
    mc = mc.set_precision(MODE).train()
    opt = torch.optim.Adam(mc.parameters(), lr=lr)
    opt.zero_grad()
    loss_c = mc.forward_kld(x)
    loss_c.backward()
    grads_c = {n: (None if p.grad is None else p.grad.clone()) for n, p in mc.named_parameters()}
    opt.step()
    # the device module, one replay of the captured step
    mg = build_flow(N, L, H, nb, K, bound=dims.B, device="cpu")
    mg.load_state_dict(sd, strict=True)
    mg.p = DoubleWellLJ(dims.D, N, 1.0, dims.B, V0_list=[-10.0, -10.5], r0=1.2, k=15)
    mg = mg.cuda().set_precision(MODE).train()
    before = {n: p.detach().clone() for n, p in mg.named_parameters()}
    step = GraphedTrainStep(mg, rows, lr=lr, weight_decay=0.0, alpha=1.0, example=x.cuda())
    assert step.flat_bn is not None and AF._last_paired
    loss_g = step.step(x.cuda())
    torch.cuda.synchronize()
    np.testing.assert_allclose(loss_g.item(), loss_c.item(), rtol=2e-5)
    moved = 0
    for (n, pg), (_, pc) in zip(mg.named_parameters(), mc.named_parameters()):
        gc = grads_c[n]
        if gc is None:
            assert torch.equal(pg.detach(), before[n]), n
            continue
        np.testing.assert_allclose(pg.grad.cpu().numpy(), gc.numpy(), rtol=2e-3, atol=2e-5, err_msg=n)
        dg = (pg.detach() - before[n]).cpu().numpy()
        dc = (pc.detach() - sd[n]).numpy()
        sure = gc.abs().numpy() > 1e-3
        moved += int(sure.sum())
        np.testing.assert_allclose(dg[sure], dc[sure], rtol=2e-3, atol=2e-5 * lr, err_msg=n)
        assert np.abs(dg - dc).max(initial=0.0) <= 2 * lr * (1 + 1e-5), n
    assert moved > 0
    mg.eval()
    sd_new = {k: v.detach().cpu().clone() for k, v in mg.state_dict().items()}
    oracle_close(mg.log_prob(x.cuda()).cpu().numpy(), OF.log_prob(sd_new, x.clone(), dims).numpy())


# --- 7. the driver -----------------------------------------------------------------------
def _driver_model(dims, kw, sd):
    m = flow_from_state_dict(sd, dims.N, bound=dims.B, **kw).set_precision(MODE)
    m.p = DoubleWellLJ(dims.D, dims.N, 1.0, dims.B, V0_list=[-10.0, -10.5], r0=1.2, k=15)
    m.q0.device = torch.device("cuda")
    return m


def test_algorithm2_trains_a_general_mode_flow():
    """Algorithm2 with a flow at (N, L, H, nb, K) = (16, 3, 40, 1, 7) in the general mode, as
    the smallest case of tests/test_gpu_algorithm2.py: two cycles with the graphed step on the
    shared launches, finite losses, sampling through bmc.step() afterwards.

    The eager epoch (graphed=False) is run from each cycle's own start (the same weights and
    training set, the same host seed for the batch order): a captured step and an eager one
    take reverse_kld's base draws from different generator offsets, which at ALPHA = 1 reach
    only the BatchNorm running statistics, and through the refeed's acceptances the next
    cycle's training set; a second run of the whole driver would train on other data from
    cycle 2 on.  Per-cycle mean losses within rtol 1e-4."""
    N, runs = 16, 100
    kw = dict(L=3, H=40, nb=1, K=7)
    dims = OF.FlowDims(N=N, B=half_box(N), **kw)
    sd = OF.random_state_dict(dims, seed=29, final_std=0.05)
    m = _driver_model(dims, kw, sd)
    box = 2 * dims.B
    rng = np.random.default_rng(4)
    init = np.mod(OP.fcc_lattice(N)[None] + rng.normal(0, 0.05, (runs, N, 2)), box)
    bmc = BatchedMonteCarlo(None, init, Physics(box), [42 + i for i in range(runs)], device="cuda",
                            initial_max_displacement=0.65)
    bmc.local_moves(500, adjust_every=100)
    alg = Algorithm2(bmc, m, batch_size=256, alpha=1.0, sampling_frequency=10, update_num_samples=1000,
                     graphed=True)
    assert alg.graphed
    for cycle in range(2):
        alg.production()
        start = {k: v.detach().clone() for k, v in m.state_dict().items()}
        torch.manual_seed(100 + cycle)
        loss = alg.train()
        assert np.isfinite(loss)
        assert alg._step.flat_bn is not None and AF._last_paired
        twin = _driver_model(dims, kw, start)
        eager = Algorithm2(type("E", (), {"C": runs})(), twin, batch_size=256, alpha=1.0, graphed=False)
        eager.training_data = alg.training_data
        torch.manual_seed(100 + cycle)
        np.testing.assert_allclose(loss, eager.train(), rtol=1e-4)
        acc, p = alg.refeed()
        assert 0.0 <= p <= 1.0
    bmc.step()
    bmc.check_errors()
