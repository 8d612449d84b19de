"""reverse_kld with gradients on the fused coupling kernels (ALPHA < 1): sample_step_grad
(fs_coupling_sample_pre / _post forward, fs_coupling_sample_bwd_post / _pre / _step backward,
csrc/spline_autograd.hip) against coupling_sample over torch ops, against the reference's own
reverse-KLD gradients (tests/golden/train.npz), inside GraphedTrainStep, and the loss head
fs_kld_loss_mix.  Bounds are those of the density direction's twins
(tests/test_gpu_train_fused.py, test_gpu_general_train.py, test_gpu_train.py,
test_gpu_train_graph.py)."""
import copy
import os

import numpy as np
import pytest
import torch

from flowstate.normflows import autograd_flow as AF
from flowstate.normflows.train import GraphedTrainStep
from test_gpu_general_train import general_layer
from test_gpu_paired import _model
from test_gpu_train_fused import a2_layer, close
from test_train_cpu import build

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture
def af_switches():
    """Restores the module switches a test flips."""
    prev = AF._fused_sample_grad, AF._sample_bwd_step, AF._force_any_k
    yield
    AF._fused_sample_grad, AF._sample_bwd_step, AF._force_any_k = prev
    AF._nan_flags.clear()


def _rows(layer, rows, seed):
    """Rows inside the tails, some with coordinates outside [-B, B] in both halves (even and odd
    columns are the identity and transform features, before and after the half-roll)."""
    B, D = layer.tail_bound, layer.num_input_channels
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = (torch.rand(rows, D, device="cuda", generator=g) * 2 - 1) * B
    z[:3, 0:2] = B * 1.5
    z[1:4, D - 2:] = -B * 1.2
    return z, torch.randn(rows, device="cuda", generator=g), g


def _buffers_close(layer, ref):
    for (n, b1), (_, b2) in zip(layer.named_buffers(), ref.named_buffers()):
        if b1.dtype == torch.int64:
            assert torch.equal(b1, b2), n
        else:
            close(b1, b2, 1e-5, n)


# (N, K, H, rows, general mode): A2's layer; ragged rows; n = 100 (the lane loop's second pass,
# D = 200 in the LDS row); K = 32; an uninstantiated K on the runtime-K kernels
SHAPES = [(64, 15, 128, 256, False), (3, 8, 32, 37, False), (100, 5, 32, 5, False), (4, 32, 32, 19, False),
          (16, 10, 96, 37, True)]


@pytest.mark.parametrize("N,K,H,rows,general", SHAPES, ids=str)
@pytest.mark.parametrize("with_lq,z_grad", [(True, True), (False, False)], ids=["lq-zgrad", "nolq-znograd"])
def test_sample_step_grad_matches_torch_ops(N, K, H, rows, general, with_lq, z_grad):
    """sample_step_grad against coupling_sample over torch ops and the element-wise spline
    (at K = 10: its runtime-K form): outputs, log q, input and parameter gradients, BatchNorm
    buffers; lq_in = None and an input that needs no gradient."""
    layer = general_layer(7, N, H, K) if general else a2_layer(7, N=N, K=K, H=H)
    ref = copy.deepcopy(layer)
    layer.train()
    ref.train()
    z, lq0, g = _rows(layer, rows, 3)
    if not with_lq:
        lq0 = None
    z1 = z.clone().requires_grad_(z_grad)
    z2 = z.clone().requires_grad_(z_grad)
    assert AF.fused_coupling_ok(layer, z1)
    assert AF._coupling_desc(layer, rows).any_k == int(general)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    before = AF.sample_grad_steps
    o1, lq1 = AF.sample_step_grad(layer, z1, lq0, flag)
    assert AF.sample_grad_steps == before + 1
    o2, ld2 = AF.coupling_sample(ref, z2)
    lq2 = (lq0 if with_lq else 0) - ld2
    close(o1, o2, 1e-5, "z")
    close(lq1, lq2, 1e-5, "log q")
    go = torch.randn(o1.shape, device="cuda", generator=g)
    gl = torch.randn(rows, device="cuda", generator=g)
    ((o1 * go).sum() + (lq1 * gl).sum()).backward()
    ((o2 * go).sum() + (lq2 * gl).sum()).backward()
    AF.check_nan_flags()
    assert int(flag.item()) == 0
    assert not AF._pending_sample_bwd
    if z_grad:
        close(z1.grad, z2.grad, 1e-4, "z grad")
    else:
        assert z1.grad is None
    for (n, p1), (_, p2) in zip(layer.named_parameters(), ref.named_parameters()):
        if p2.grad is None:
            assert p1.grad is None or not p1.grad.abs().max().item(), n
            continue
        close(p1.grad, p2.grad, 1e-4, n)
    _buffers_close(layer, ref)


@pytest.mark.parametrize("N,K,H,rows,general", SHAPES[1:], ids=str)
def test_forward_under_grad_equals_sample_step(N, K, H, rows, general):
    layer = general_layer(8, N, H, K) if general else a2_layer(8, N=N, K=K, H=H)
    ref = copy.deepcopy(layer)
    layer.train()
    ref.train()
    z, lq0, _ = _rows(layer, rows, 4)
    f1 = torch.zeros(1, dtype=torch.int32, device="cuda")
    f2 = torch.zeros(1, dtype=torch.int32, device="cuda")
    o1, lq1 = AF.sample_step_grad(layer, z.clone().requires_grad_(True), lq0, f1)
    with torch.no_grad():
        o2, lq2 = AF.sample_step(ref, z.clone(), lq0, f2)
    assert o1.requires_grad and lq1.requires_grad
    assert torch.equal(o1, o2) and torch.equal(lq1, lq2)
    assert int(f1.item()) == int(f2.item()) == 0
    for (n, b1), (_, b2) in zip(layer.named_buffers(), ref.named_buffers()):
        assert torch.equal(b1, b2), n


def _reverse_grads(m, z):
    for p in m.parameters():
        p.grad = None
    z = z.clone().requires_grad_(True)
    loss, zs = m._reverse_kld_from(z)
    loss.backward()
    torch.cuda.synchronize()
    assert not AF._pending_sample_bwd
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    grads["z"] = z.grad.clone()
    return loss.detach().clone(), zs.detach().clone(), grads


@pytest.mark.parametrize("N,kw,rows", [(16, dict(L=2, H=32, nb=1, K=8), 37), (100, dict(L=2, H=32, nb=1, K=5), 5),
                                       (3, dict(L=3, H=40, nb=1, K=7), 19)], ids=["n16", "n100", "n3-k7-general"])
def test_fused_backward_launch_equals_separate_launches(N, kw, rows, af_switches):
    """fs_coupling_sample_bwd_step (layer l's bwd_pre + layer l - 1's bwd_post on the row in
    LDS) against the separate launches: the same row functions, so every gradient is equal."""
    outs = []
    for fused in (True, False):
        AF._sample_bwd_step = fused
        m = _model(N, kw, seed=5)
        if kw["K"] not in AF._HIP_K:
            m.set_precision("f32-general")
        z = m.q0(rows).cuda()
        z[::3, ::5] *= 1.2  # beyond the bound: the identity branches
        n0 = AF.sample_bwd_steps
        outs.append(_reverse_grads(m, z))
        assert AF.sample_bwd_steps - n0 == ((kw["L"] - 1) if fused else 0)
    (la, za, ga), (lb, zb, gb) = outs
    assert torch.equal(la, lb) and torch.equal(za, zb)
    assert ga.keys() == gb.keys() and len(ga) > 10
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


@pytest.mark.parametrize("K", [5, 8, 15, 32])
def test_runtime_k_backward_matches_instantiated(K, af_switches):
    """reverse_kld and its backward with every coupling launch forced onto the runtime-K
    kernels (AF._force_any_k) against the instantiated ones, with the comparison
    test_runtime_k_kernels_match_instantiated applies to the density twins."""
    N, kw, rows = 16, dict(L=3, H=32, nb=1, K=K), 37
    outs = []
    for force in (False, True):
        AF._force_any_k = force
        m = _model(N, kw, seed=2)
        assert AF._coupling_desc(m.flows[0], rows).any_k == int(force)
        torch.cuda.manual_seed(13)
        z = m.q0(rows).cuda()
        z[::7, ::5] *= 1.2
        loss, _, grads = _reverse_grads(m, z)
        outs.append((loss, grads, {n: b.clone() for n, b in m.named_buffers()}))
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


def test_reverse_kld_gradients_match_reference():
    """reverse_kld(64) and its gradients on the fused path against the reference's
    (tests/golden/train.npz rkld, rkld_z, gr/*), test_gpu_train.py's bounds; every layer took
    sample_step_grad."""
    m, f = build("cuda")
    names = [str(n) for n in f["names"]]
    before = AF.sample_grad_steps
    lr_, zr = m.reverse_kld(64)
    assert AF.sample_grad_steps - before == len(m.flows)
    np.testing.assert_allclose(lr_.item(), float(f["rkld"]), rtol=2e-5)
    np.testing.assert_allclose(zr.detach().cpu().numpy(), f["rkld_z"], rtol=1e-5, atol=5e-4)
    gr = torch.autograd.grad(lr_, list(m.parameters()), allow_unused=True)
    assert not AF._pending_sample_bwd
    checked = 0
    for n, g in zip(names, gr):
        ref = f["gr/" + n]
        if ref.size == 0:
            continue
        scale = max(1.0, float(np.abs(ref).max()))
        np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=2e-3, atol=2e-5 * scale, err_msg=n)
        checked += 1
    assert checked > 10


def _eager(m, opt, x, alpha):
    opt.zero_grad()
    e, _ = m.reverse_kld(64)
    s = m.forward_kld(x)
    loss = alpha * s + (1 - alpha) * e
    if bool(~(torch.isnan(loss) | torch.isinf(loss))):
        loss.backward()
        opt.step()
    return loss


def test_graphed_step_at_alpha_half_matches_eager():
    """GraphedTrainStep(alpha=0.5) on the fused sampling-pass backward against the eager
    reference loop (test_graphed_step_matches_eager's bounds), then a NaN batch: nothing the
    optimizer owns may move."""
    alpha, lr, wd = 0.5, 5e-3, 1e-4
    m1, f = build("cuda")
    m2, _ = build("cuda")
    x = torch.from_numpy(f["x"]).cuda()
    opt = torch.optim.Adam(m1.parameters(), lr=lr, weight_decay=wd)
    before = AF.sample_grad_steps
    g = GraphedTrainStep(m2, 64, lr, wd, alpha=alpha, example=x)
    assert AF.sample_grad_steps > before  # the captured step ran the new path
    p0 = {k: v.clone() for k, v in m1.state_dict().items()}
    for sd1, sd2 in zip(m1.state_dict().values(), m2.state_dict().values()):
        assert torch.equal(sd1, sd2)  # capture left the model untouched
    for i in range(4):
        xb = x.roll(i, 0)
        l1 = _eager(m1, opt, xb, alpha)
        l2 = g.step(xb)
        np.testing.assert_allclose(l2.item(), l1.item(), rtol=1e-4)
    for (k, v1), v2 in zip(m1.state_dict().items(), m2.state_dict().values()):
        if not v1.is_floating_point():
            assert torch.equal(v1, v2), k
            continue
        moved = (v1 - p0[k]).norm().item()
        diff = (v2 - v1).norm().item()
        assert diff <= 2e-2 * moved + 1e-6, (k, diff, moved)
    keep = {k: v.clone() for k, v in m2.state_dict().items() if "running" not in k and "num_batches" not in k}
    bad = x.clone()
    bad[0, 0] = float("nan")
    loss = g.step(bad)
    assert torch.isnan(loss).item()
    for k, v in keep.items():
        assert torch.equal(m2.state_dict()[k], v), k


@pytest.mark.parametrize("B,R", [(1, 1), (257, 257)])
@pytest.mark.parametrize("alpha", [0.0, 0.3, 1.0])
def test_kld_loss_mix_head(B, R, alpha):
    """fs_kld_loss_mix / _backward (autograd_flow._KldLossMix) against the torch expression:
    the value within float32 rounding of the sums, the three gradients (exact products) equal."""
    g = torch.Generator(device="cuda").manual_seed(B + int(10 * alpha))
    lq = torch.randn(B, device="cuda", generator=g) * 3 - 40
    E = torch.randn(R, device="cuda", generator=g) * 5 + 20
    lr_ = torch.randn(R, device="cuda", generator=g) * 3 - 35
    a = [t.clone().requires_grad_(True) for t in (lq, E, lr_)]
    b = [t.clone().requires_grad_(True) for t in (lq, E, lr_)]
    got = AF.kld_loss_mix(*a, alpha)
    assert type(got.grad_fn).__name__ == "_KldLossMixBackward"
    want = alpha * (-torch.mean(b[0])) + (1 - alpha) * (torch.mean(b[1]) + torch.mean(b[2]))
    torch.testing.assert_close(got, want, rtol=1e-6, atol=0)
    seed = torch.tensor(1.7, device="cuda")
    got.backward(seed)
    want.backward(seed)
    for x1, x2, n in zip(a, b, ("log_q", "energy", "lq_rev")):
        assert torch.equal(x1.grad, x2.grad), (n, x1.grad[0].item(), x2.grad[0].item())


def test_sampling_backward_launch_census():
    """reverse_kld and its backward on an L = 3 stack: no element-wise spline launches, one
    separate bwd_post (the last layer's), two fused launches between layers, one separate
    bwd_pre (the first layer's)."""
    from torch.profiler import ProfilerActivity, profile

    N, rows = 16, 64
    m = _model(N, dict(L=3, H=64, nb=2, K=8))
    z = m.q0(rows).cuda()
    loss, _ = m._reverse_kld_from(z)  # warm-up: allocator, module load
    loss.backward()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        loss, _ = m._reverse_kld_from(z)
        loss.backward()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    if not names:
        pytest.skip("the profiler recorded no device kernels")
    assert not [n for n in names if "rqs_forward" in n or "rqs_backward" in n]
    assert sum("coupling_sample_bwd_post" in n for n in names) == 1, names
    assert sum("coupling_sample_bwd_step" in n for n in names) == 2, names
    assert sum("coupling_sample_bwd_pre" in n for n in names) == 1, names
    assert sum("coupling_sample_pre" in n for n in names) == 3, names


def _epoch(alpha):
    from flowstate.algorithm2 import Algorithm2
    from test_algorithm2_cpu import _model as cycle_model
    from test_gpu_algorithm2 import _NoEngine

    f = np.load(os.path.join(G, "train_cycle.npz"))
    m = cycle_model().cuda()  # built on the CPU and moved: q0 draws from the CPU default generator
    p0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    a = Algorithm2(_NoEngine(), m, batch_size=256, alpha=alpha, graphed=False)
    a.training_data = torch.tensor(f["data"], dtype=torch.float32).reshape(600, -1).cuda()
    torch.manual_seed(23)
    avg = a.train()
    return f, m, p0, avg


def test_training_epoch_at_alpha_half_matches_reference(af_switches):
    """One Algorithm-2 epoch at ALPHA = 0.5 on the device against the reference's
    (tests/golden/train_cycle.npz, tag a5), test_graphed_training_epoch_matches_reference's
    bounds; first on the per-op path (the switch off), then on the fused one."""
    for fused in (False, True):
        AF._fused_sample_grad = fused
        before = AF.sample_grad_steps
        f, m, p0, avg = _epoch(0.5)
        assert (AF.sample_grad_steps > before) == fused
        np.testing.assert_allclose(avg, float(f["a5_avg"]), rtol=1e-4, err_msg=f"fused={fused}")
        for k, v in m.state_dict().items():
            if "running" in k or not v.is_floating_point():
                continue
            ref = torch.from_numpy(f["a5/" + k]).cuda()
            moved = (ref - p0[k]).norm().item()
            assert (v - ref).norm().item() <= 3e-2 * moved + 1e-6, (k, fused)
