"""The general-shape flow mode ("f32-general", fs_flow_dims.precision 4:
csrc/flow_general_kernels.hip) on the MI355X: density, sampling and proposal passes at
hidden widths and bin counts no instantiated kernel covers, against the oracle with the
bounds of tests/test_gpu_flow.py; row independence; an A/B against the instantiated
kernels at shapes both cover; the fused MH step; the runtime-K training spline
(fs_rqs_forward_any / fs_rqs_backward_any) and a training step in this mode."""
import functools

import numpy as np
import pytest
import torch

from flowstate import _lib
from flowstate.MCMC import BatchedMonteCarlo, Physics
from flowstate.models import build_flow, flow_from_state_dict, half_box
from flowstate.normflows import autograd_flow as AF
from oracle import flow as OF
from oracle import physics as OP
from test_gpu_flow import close

pytestmark = pytest.mark.gpu

MODE = "f32-general"
# (N, L, H, nb, K)
SHAPES = [(3, 2, 24, 1, 7),      # H < 32, odd K, D = 6
          (3, 3, 40, 0, 10),     # H not a tile multiple, no residual block, odd L
          (15, 2, 96, 2, 16),    # odd N, H = 96
          (4, 2, 48, 3, 1),      # K = 1
          (64, 2, 100, 1, 20),   # N = 64 with padded H
          (64, 1, 320, 1, 31),   # H > 256 (32 rows per workgroup), K = 31
          (64, 2, 512, 1, 32)]   # the upper corner
AB_SHAPES = [(16, 3, 64, 2, 8), (3, 2, 32, 2, 5)]  # instantiated: both modes run them
ROWS = 200


@functools.lru_cache(maxsize=None)
def case(shape):
    """Weights, inputs and the oracle's results of one shape, computed once and read only."""
    N, L, H, nb, K = shape
    dims = OF.FlowDims(N=N, L=L, H=H, nb=nb, K=K, B=half_box(N))
    sd = OF.random_state_dict(dims, seed=7)
    g = torch.Generator().manual_seed(31 + H)
    x = (torch.rand((ROWS + 2, dims.D), generator=g) * 2 - 1) * dims.B
    x[ROWS, 0] = dims.B * 1.25  # a coordinate outside the box: log q = -inf
    x[ROWS + 1, dims.D - 1] = -dims.B * 1.01
    z0 = (torch.rand((ROWS, dims.D), generator=g) * 2 - 1) * dims.B
    lq, z, _ = OF.log_prob(sd, x.clone(), dims, per_layer=True)
    xs, ld = OF.sample_from(sd, z0.clone(), dims, with_logdet=True)
    ref = dict(x=x, z0=z0, lq=lq.numpy(), z=z.numpy(), xs=xs.numpy(), ld=ld.numpy())
    return dims, sd, ref


def model_of(shape, mode=MODE):
    dims, sd, _ = case(shape)
    N, L, H, nb, K = shape
    return flow_from_state_dict(sd, N, L, H, nb, K, bound=dims.B).set_precision(mode)


def check_against_oracle(m, shape):
    """The bounds of test_gpu_flow.py:39-54 on log_prob, inverse and forward."""
    dims, _, ref = case(shape)
    x = ref["x"].cuda()
    close(m.log_prob(x).cpu().numpy(), ref["lq"])
    assert np.isneginf(ref["lq"][ROWS:]).all() and np.isfinite(ref["lq"][:ROWS]).all()
    z = m.inverse(x[:ROWS]).cpu().numpy()
    np.testing.assert_allclose(z, ref["z"][:ROWS], rtol=0, atol=2e-4 * dims.B)
    xs, ld = m.forward_and_log_det(ref["z0"].cuda())
    np.testing.assert_allclose(xs.cpu().numpy(), ref["xs"], rtol=0, atol=5e-4 * dims.B)
    close(ld.cpu().numpy(), ref["ld"], rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_general_mode_matches_oracle(shape):
    check_against_oracle(model_of(shape), shape)


@pytest.mark.parametrize("shape", SHAPES[:3], ids=str)
def test_default_mode_refuses_these_shapes(shape):
    """What the general mode is for: the same model in the default mode raises."""
    m = model_of(shape, "f32")
    with pytest.raises(_lib.FlowStateError, match="unsupported"):
        m.log_prob(case(shape)[2]["x"].cuda())


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[5]], ids=str)
def test_rows_are_independent_of_batch_and_position(shape):
    """A row's log q and sample are bit-identical whatever the batch size and the row's
    position (64 rows per workgroup at H = 96, 32 at H = 320)."""
    _, _, ref = case(shape)
    m = model_of(shape)
    x, z0 = ref["x"][:ROWS].cuda(), ref["z0"].cuda()
    lq = m.log_prob(x)
    xs, ld = m.forward_and_log_det(z0)
    for lo, hi in ((0, 1), (0, 65), (0, 200), (135, 200), (199, 200), (31, 64)):
        assert torch.equal(m.log_prob(x[lo:hi]), lq[lo:hi]), (lo, hi)
        xs2, ld2 = m.forward_and_log_det(z0[lo:hi])
        assert torch.equal(xs2, xs[lo:hi]) and torch.equal(ld2, ld[lo:hi]), (lo, hi)
    assert m.log_prob(x[:0]).numel() == 0


def _propose(m, dims, C, seed, counter, row_offset):
    lib, p = _lib.load(), _lib.ptr
    cfg = torch.empty((C, dims.D), device="cuda")
    cen = torch.empty_like(cfg)
    xo = torch.empty_like(cfg)
    lq = torch.empty(C, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.fs_flow_propose_lq(m.dims(), p(m.packed()), C, seed, counter, row_offset, float(dims.B), p(cfg),
                                      p(cen), p(xo), p(lq), p(err), _lib.stream_ptr()), "fs_flow_propose_lq")
    assert int(err.item()) == 0
    return cfg, cen, xo, lq


@pytest.mark.parametrize("shape", AB_SHAPES, ids=str)
def test_general_mode_against_instantiated_kernels(shape):
    """The same weights in "f32" and "f32-general": both within the oracle's bounds, and the
    proposal pass draws the same Philox stream (equal seed, counter, row offset)."""
    dims, _, _ = case(shape)
    tuned, general = model_of(shape, "f32"), model_of(shape)
    check_against_oracle(tuned, shape)
    check_against_oracle(general, shape)
    C = 200
    a = _propose(tuned, dims, C, 3, 5, 1000)
    b = _propose(general, dims, C, 3, 5, 1000)
    np.testing.assert_allclose(b[0].cpu().numpy(), a[0].cpu().numpy(), rtol=0, atol=5e-4 * dims.B)
    # config = fl32(x + B), centered = fl32(config - half_width), in this mode too
    assert torch.equal(b[0], b[2] + float(np.float32(dims.B)))
    assert torch.equal(b[1], (b[0].double() - float(dims.B)).float())
    # the launch's own log q is the density pass's on its proposals
    close(b[3].cpu().numpy(), general.log_prob(b[1]).cpu().numpy(), rtol=1e-4, atol=1e-3)
    # rows keyed by their global index: a shard starting at row 100 draws rows 100.. of the whole
    c = _propose(general, dims, 50, 3, 5, 1100)
    assert torch.equal(c[0], b[0][100:150]) and torch.equal(c[3], b[3][100:150])


def test_fused_mh_step_in_general_mode():
    from test_gpu_mh import _fused_vs_oracle

    flips, rule, acc, n = _fused_vs_oracle(16, dict(L=3, H=96, nb=1, K=10), C=512, steps=4, precision=MODE)
    assert rule == 0
    assert flips <= max(1, n // 2000), (flips, n)


def test_multi_step_launch_matches_single_steps_in_general_mode():
    """step(3) (one proposal launch of 3 C rows, fs_nf_mh_steps) leaves every chain exactly
    where three step() calls do, bit for bit (tests/test_gpu_mh.py:313-340 in this mode)."""
    N, C = 16, 512
    dims_kw = dict(L=3, H=96, nb=1, K=10)
    dims = OF.FlowDims(N=N, B=half_box(N), **dims_kw)
    sd = OF.random_state_dict(dims, seed=6)
    model = flow_from_state_dict(sd, N, bound=dims.B, **dims_kw).set_precision(MODE)
    L = float(np.sqrt(N / 0.03))
    rng = np.random.default_rng(4)
    init = np.mod(OP.fcc_lattice(N)[None] + rng.normal(0, 0.05, (C, N, 2)), L)
    seeds = np.arange(42, 42 + C, dtype=np.uint64)
    multi = BatchedMonteCarlo(model, init, Physics(L, L), seeds, chain_offset=1000)
    single = BatchedMonteCarlo(model, init, Physics(L, L), seeds, chain_offset=1000)
    single.MAX_STEPS_PER_LAUNCH = 1
    assert multi.steps_per_launch() > 1 and single.steps_per_launch() == 1
    multi.step(3)
    for _ in range(3):
        single.step()
    for name in ("state", "E_old", "W_old", "nll_old", "pcg", "accept", "attempts", "accepted", "n_accept"):
        assert torch.equal(getattr(multi, name), getattr(single, name)), name
    assert multi.step_count == single.step_count == 3
    assert int(multi.accepted.sum().item()) > 0
    multi.check_errors()


def _spline_case(K, inverse, M=4096):
    g = torch.Generator().manual_seed(K + 7 * int(inverse))
    B = 3.0
    x = (torch.rand(M, generator=g) * 2 - 1) * B * 1.05  # ~5 % outside
    x[:4] = torch.tensor([B, -B, 0.0, B * 1.2])
    uw = torch.randn(M, K, generator=g) * 0.7
    uh = torch.randn(M, K, generator=g) * 0.7
    ud = torch.randn(M, K + 1, generator=g) * 0.7
    ud[:8, 0] = 25.0  # softplus above its threshold
    wo = torch.randn(M, generator=g)
    wl = torch.randn(M, generator=g)
    return B, x, uw, uh, ud, wo, wl


def _spline_close(got, want):
    """test_gpu_spline_grad's tolerance: element-wise, at most 4 ill-conditioned rows."""
    names = ["out", "lad", "g_x", "g_uw", "g_uh", "g_ud"]
    for n, a, b in zip(names, got, want):
        a, b = a.numpy().reshape(len(a), -1), b.numpy().reshape(len(b), -1)
        scale = max(1.0, float(np.abs(b).max()))
        bad = ~np.isclose(a, b, rtol=2e-4, atol=2e-5 * scale)
        rows = np.nonzero(bad.any(1))[0]
        assert len(rows) <= 4, (n, len(rows), a[rows[:3]], b[rows[:3]])
        np.testing.assert_allclose(a, b, rtol=5e-2, atol=5e-3 * scale, err_msg=n)


@pytest.mark.parametrize("K", [1, 7, 10, 20, 31])
@pytest.mark.parametrize("inverse", [False, True])
def test_runtime_k_spline_matches_torch(K, inverse):
    B, x, uw, uh, ud, wo, wl = _spline_case(K, inverse)
    res = {}
    for dev in ("cuda", "cpu"):
        ts = [t.to(dev).clone().requires_grad_(True) for t in (x, uw, uh, ud)]
        if dev == "cuda":
            out, lad = AF.circular_rqs(*ts, B, inverse, any_k=True)
        else:
            out, lad = AF.circular_rqs_torch(*ts, B, inverse)
        loss = (out * wo.to(dev)).sum() + (lad * wl.to(dev)).sum()
        grads = torch.autograd.grad(loss, ts)
        res[dev] = [out.detach().cpu(), lad.detach().cpu()] + [gr.cpu() for gr in grads]
    AF.check_nan_flags()
    _spline_close(res["cuda"], res["cpu"])


def test_runtime_k_spline_still_raises_without_any_k():
    uw = torch.zeros(4, 10, device="cuda")
    with pytest.raises(_lib.FlowStateError, match="K=10"):
        AF.circular_rqs(torch.zeros(4, device="cuda"), uw, uw, torch.zeros(4, 11, device="cuda"), 3.0, False)


@pytest.mark.parametrize("K", [1, 7, 10, 20, 31])
def test_runtime_k_spline_forward_inverse_consistent(K):
    torch.manual_seed(K)
    shape, B = (2, 3, 4), 3.0
    uw = torch.randn(*shape, K, device="cuda")
    uh = torch.randn(*shape, K, device="cuda")
    ud = torch.randn(*shape, K + 1, device="cuda")
    x = torch.randn(*shape, device="cuda") * 2  # some outside [-B, B]: identity, log-det 0
    y, ld = AF.circular_rqs(x, uw, uh, ud, B, inverse=False, any_k=True)
    x2, ld2 = AF.circular_rqs(y, uw, uh, ud, B, inverse=True, any_k=True)
    AF.check_nan_flags()
    torch.testing.assert_close(x2, x, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(ld + ld2, torch.zeros_like(ld), atol=1e-3, rtol=1e-3)
    out = x.abs() > B
    assert torch.equal(y[out], x[out]) and torch.equal(ld[out], torch.zeros_like(ld[out]))


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("K", [5, 8, 15, 32])
def test_runtime_k_entry_points_match_instantiated_kernels(K, inverse):
    """Every instantiated K through fs_rqs_forward_any / fs_rqs_backward_any against fs_rqs_forward /
    fs_rqs_backward on the same operands (M = 1000: a ragged last workgroup)."""
    B, x, uw, uh, ud, wo, wl = (t.cuda() if torch.is_tensor(t) else t for t in _spline_case(K, inverse, M=1000))
    lib, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
    M = x.numel()
    res = {}
    for name, fwd, bwd in (("any", lib.fs_rqs_forward_any, lib.fs_rqs_backward_any),
                           ("inst", lib.fs_rqs_forward, lib.fs_rqs_backward)):
        out, lad, gx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        guw, guh, gud = torch.empty_like(uw), torch.empty_like(uh), torch.empty_like(ud)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(fwd(M, K, int(inverse), p(x), p(uw), p(uh), p(ud), B, p(out), p(lad), p(flag), st), name)
        _lib.check(bwd(M, K, int(inverse), p(x), p(uw), p(uh), p(ud), B, p(wo), p(wl), p(gx), p(guw), p(guh), p(gud),
                       st), name)
        assert int(flag.item()) == 0
        res[name] = [t.cpu() for t in (out, lad, gx, guw, guh, gud)]
    _spline_close(res["any"], res["inst"])


def test_training_step_in_general_mode():
    """forward_kld + backward on the device in "f32-general" at an uninstantiated shape
    against the same module on the CPU (torch restatement), bounds of test_gpu_train.py:15;
    after one Adam step the general-mode log_prob matches the oracle on the new weights."""
    shape = (3, 2, 40, 1, 7)
    N, L, H, nb, K = shape
    dims = OF.FlowDims(N=N, L=L, H=H, nb=nb, K=K, B=half_box(N))
    sd = OF.random_state_dict(dims, seed=7, final_std=0.05)
    g = torch.Generator().manual_seed(2)
    x = (torch.rand((64, dims.D), generator=g) * 2 - 1) * dims.B
    res = {}
    for dev in ("cuda", "cpu"):
        m = build_flow(N, L, H, nb, K, bound=dims.B, device="cpu")
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).set_precision(MODE).train()
        loss = m.forward_kld(x.to(dev))
        grads = torch.autograd.grad(loss, list(m.parameters()), allow_unused=True)
        res[dev] = (m, loss.item(), grads)
    m, loss, grads = res["cuda"]
    _, loss_c, grads_c = res["cpu"]
    np.testing.assert_allclose(loss, loss_c, rtol=2e-5)
    for (n, _), a, b in zip(m.named_parameters(), grads, grads_c):
        if b is None:
            assert a is None or not a.abs().max().item(), n
            continue
        np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=2e-3, atol=2e-5, err_msg=n)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    opt.zero_grad()
    m.forward_kld(x.cuda()).backward()
    opt.step()
    m.eval()
    sd_new = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert not torch.equal(sd_new["flows.0.prqct.transform_net.final_layer.weight"],
                           sd["flows.0.prqct.transform_net.final_layer.weight"])
    close(m.log_prob(x.cuda()).cpu().numpy(), OF.log_prob(sd_new, x.clone(), dims).numpy())
