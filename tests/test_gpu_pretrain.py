"""Algorithm 1's pretraining stage on the MI355X: the forward-only HIP-graph step
(GraphedTrainStep(..., reverse=False)) and flowstate.algorithm1.pretrain's graphed epochs
against the eager loop, the reference's own step on A1's conditioner
(tests/golden/pretrain_a1.npz), the skip rules and the written model file."""
import numpy as np
import pytest
import torch

from test_pretrain_cpu import build_pretrain_a1, check_pretrain_files, check_pretrain_step, rows, small_flow

pytestmark = pytest.mark.gpu

MID = dict(L=2, H=64, nb=2, K=8)


def test_graphed_pretraining_matches_eager():
    """40 rows, batch 16 (tail of 8: two captured graphs), 2 epochs, two models from one
    state dict under one seed: graphed epochs against the eager reference loop.  Bounds and
    reasoning of test_gpu_train_graph.test_graphed_step_matches_eager: per step the loss to
    rtol 1e-4; per tensor |p_graphed - p_eager| <= 2e-2 |p_eager - p_0| + 1e-6 (Adam
    normalises each coordinate, so float32 noise on a near-zero gradient is an lr-sized
    difference on that coordinate: the updates are compared per tensor in norm).  As there,
    the run has a weight decay of 1e-4: each block's first bias sits in front of a train-mode
    BatchNorm, whose batch mean removes it, so its true gradient is exactly zero and what
    either path computes is rounding noise of ~1e-9; with weight_decay = 0 Adam turns the
    sign of that noise into a full lr-sized step, on which no two summation orders agree
    (measured so: 1.0e-4 apart on a tensor that moved 8.4e-5), while wd p of ~1e-6 makes the
    update of those tensors determined.  weight_decay = 0, Algorithm 1's own setting, is
    checked against the reference's step in the golden test below."""
    from flowstate import algorithm1 as A1
    from flowstate.normflows.train import GraphedTrainStep

    m1, dims = small_flow(device="cuda", **MID)
    m2, _ = small_flow(device="cuda", **MID)
    m3, _ = small_flow(device="cuda", **MID)
    x = rows(40, dims.B)
    p0 = {k: v.clone() for k, v in m1.state_dict().items()}
    # the step itself: a model without a target, left untouched by the capture
    assert m3.p is None
    g = GraphedTrainStep(m3, 16, 1e-3, 0.0, example=x[:16].cuda(), extra_batch_sizes=(8,), reverse=False)
    assert sorted(g.graphs) == [8, 16] and g.flat_bn is not None and g._fused_adam_ok()
    for (k, v), w in zip(p0.items(), m3.state_dict().values()):
        assert torch.equal(v, w), k
    torch.manual_seed(21)
    eager = A1.pretrain(m1, x, epochs=2, batch_size=16, lr=1e-3, weight_decay=1e-4, graphed=False)
    torch.manual_seed(21)
    graphed = A1.pretrain(m2, x, epochs=2, batch_size=16, lr=1e-3, weight_decay=1e-4)
    assert graphed.graphed and not eager.graphed
    assert graphed.skipped == 0 and graphed.adam_steps == eager.adam_steps == 6
    assert graphed.loss_hist.dtype == np.float64 and graphed.loss_hist.shape == (6,)
    np.testing.assert_allclose(graphed.loss_hist, eager.loss_hist, rtol=1e-4)
    np.testing.assert_allclose(graphed.loss_epoch, eager.loss_epoch, rtol=1e-4)
    for (k, v1), v2 in zip(m1.state_dict().items(), m2.state_dict().values()):
        if not v1.is_floating_point():
            assert torch.equal(v1, v2), k
            continue
        moved = (v1 - p0[k]).norm().item()
        diff = (v2 - v1).norm().item()
        assert diff <= 2e-2 * moved + 1e-6, (k, diff, moved)


def test_graphed_pretraining_step_matches_reference_on_a1_conditioner():
    """One graphed forward-only step at batch 512 (16 row tiles) on A1's own conditioner
    (H=256, 32 blocks, K=32; L=2: the smallest depth with an inter-layer backward hand-off)
    against the reference's own step: the loss, every gradient as a multiple of the
    reference's own float32 error against float64, the running statistics, Adam's update.
    Bounds: test_pretrain_cpu.PRETRAIN_TOL (1.5 x gradients, 2 x update, the Algorithm-2
    test's).  Measured (also in DESIGN.md, "Algorithm-1 pretraining"): whole-tensor gradients
    0.22-1.72 x the reference's float32 error in 2-norm (1.93 x in max-abs), per-tensor norms
    0.81 x, Adam update 2.36 x.  The large tensors are closer to float64 than the reference
    is (initial weights 0.22 x / 0.47 x, final bias 0.41 x).  1.72 x is the residual stream's
    bias gradients (initial_layer.bias, blocks.*.linear_layers.1.bias: all one column sum of
    the stream's gradient, since every block's branch starts with a BatchNorm whose backward
    has a zero column sum), 3.6e-7 against the reference's 2.1e-7 on |g| = 5.6e-2: both are
    what 32 blocks of branch gradients with a zero exact column sum leave behind in float32,
    and the device sums 512 rows in MFMA k order where torch's CPU sum is pairwise.  2.36 x is
    one BatchNorm bias (1.9e-7 against 7.9e-8 on an update of 1.6e-3, gradient 1.27 x): Adam's
    near-sign first step on its near-zero coordinates, as the 1.67 x of the Algorithm-2 test.
    Both sit under the bounds only through their absolute floors (1e-7), which are the
    Algorithm-2 test's too: findings, recorded, and no bound is widened for them."""
    from flowstate.normflows.train import GraphedTrainStep

    m, f = build_pretrain_a1("cuda")
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    x = torch.from_numpy(f["x"]).cuda()
    step = GraphedTrainStep(m, 512, float(f["lr"]), float(f["wd"]), example=x, reverse=False)
    assert step.flat_bn is not None and step.flat_bn.intact() and step._fused_adam_ok()
    assert len(step.graphs[512].keep) == 3  # the flat running-statistics snapshot, not 3 per module
    loss = step.step(x)
    torch.cuda.synchronize()
    names = {id(p): n for n, p in m.named_parameters()}
    grads = {names[id(p)]: step._flat_grad[o:o + p.numel()].view_as(p).clone()
             for p, o in zip(step.params, step._goffs)}
    worst, worst_mx, worst_n, worst_u = check_pretrain_step(m, f, loss.item(), grads, before)
    # a finding to explain, not a bound to widen (the bounds are PRETRAIN_TOL's)
    print(f"measured multiples: gradient {worst:.3f} (max-abs {worst_mx:.3f}, norms {worst_n:.3f}), "
          f"update {worst_u:.3f}")


def test_forward_only_graph_leaves_no_trace_of_a_skipped_step():
    """A batch with a NaN row: the loss is not finite, so Adam skips, and the graph puts the
    BatchNorm running statistics (updated inside the forward) back: parameters, Adam
    moments and step count, running statistics and num_batches_tracked equal their values
    before the step.  A later good step updates them all."""
    from flowstate.normflows.train import GraphedTrainStep

    m, dims = small_flow(device="cuda", **MID)
    x = rows(48, dims.B).cuda()
    g = GraphedTrainStep(m, 16, 1e-3, 0.0, example=x[:16], reverse=False)
    assert torch.isfinite(g.step(x[:16])).item()

    def state():
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        sd.update({f"adam{i}": t.clone() for i, t in enumerate(g._state_tensors[1:])})
        return sd

    s1 = state()
    assert len(g._state_tensors) == 4 and float(g._state_tensors[1]) == 1.0  # step, exp_avg, exp_avg_sq
    bad = x[16:32].clone()
    bad[3, 1] = float("nan")
    loss = g.step(bad)
    assert not torch.isfinite(loss).item()
    s2 = state()
    assert any("running_mean" in k for k in s1) and any("num_batches_tracked" in k for k in s1)
    for k, v in s1.items():
        assert torch.equal(s2[k], v), k
    assert not bool(g.nan_state())  # a non-finite loss is not the sticky spline-NaN word
    assert torch.isfinite(g.step(x[32:48])).item()
    s3 = state()
    stepped = {n for n, _ in m.named_parameters() if not n.endswith("preprocessing.weights")}
    for k, v in s2.items():
        if not (k in stepped or "running_" in k or "num_batches_tracked" in k or k.startswith("adam")):
            assert torch.equal(s3[k], v), k  # index buffers; the fork's unused weights (no gradient)
            continue
        assert not torch.equal(s3[k], v), k
        assert bool(torch.isfinite(s3[k].float()).all()), k
    # the sticky word: a set word makes every later replay write nothing at all
    g._sticky.fill_(1)
    loss, flag = g.step(x[:16], check=False)
    torch.cuda.synchronize()
    for k, v in s3.items():
        assert torch.equal(state()[k], v), k
    g.reset_nan()
    g.step(x[:16])
    assert not torch.equal(state()["adam0"], s3["adam0"])


def test_pretrained_model_file_gives_the_same_density(tmp_path):
    """After graphed pretraining the eval-mode HIP density pass sees the trained weights
    (replays bump no tensor versions) and equals that of a fresh model loaded from the
    written .pth, which holds every tensor once although the step re-homed them flat."""
    from flowstate import algorithm1 as A1

    m, dims = small_flow(device="cuda", **MID)
    x = rows(40, dims.B)
    lp0 = m.eval().log_prob(x.cuda())  # packs the initial weights
    torch.manual_seed(4)
    res = A1.pretrain(m, x.reshape(40, 3, 2).numpy(), epochs=2, batch_size=16, lr=1e-3, out_dir=str(tmp_path))
    assert res.graphed and not m.training
    lp1 = m.log_prob(x.cuda())
    assert not torch.equal(lp0, lp1)
    fresh, _ = small_flow(seed=9, **MID)
    check_pretrain_files(res, m, str(tmp_path), fresh)
    fresh = fresh.cuda().eval()
    assert torch.equal(fresh.log_prob(x.cuda()), lp1)


def _bn_in_load_product(M, K, N, lean, seed):
    """One BatchNorm-in-load forward product (fs_linear_f32_ex) on the producer's tile
    statistics of x: [y, tile statistics, a_out, mean, invstd, var, running mean / var, count]."""
    from flowstate import _lib

    L, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, K), generator=g).cuda()
    w = (torch.randn((N, K), generator=g) * 0.1).cuda()
    b = torch.randn(N, generator=g).cuda()
    gam, bet = (torch.rand(K, generator=g) + 0.5).cuda(), (torch.randn(K, generator=g) * 0.1).cuda()
    tiles = (M + 31) // 32
    xst = torch.empty((tiles, K, 2), device="cuda")
    xx = torch.empty_like(x)
    prev = L.fs_set_lean_gemm(1 if lean else 0)
    try:
        _lib.check(L.fs_linear_f32_ex(_lib.GemmF32(M, K, K, p(x), K, 1, p(torch.eye(K, device="cuda")), 1, K, None,
                                                   None, 0, p(xx), K, None), None, p(xst), st()))
        y = torch.empty((M, N), device="cuda")
        sto = torch.empty((tiles, N, 2), device="cuda")
        u = torch.empty_like(xx)
        mo, io, vo = (torch.empty(K, device="cuda") for _ in range(3))
        rm, rv = torch.zeros(K, device="cuda"), torch.ones(K, device="cuda")
        nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
        gd = _lib.GemmF32(M, N, K, p(xx), K, 1, p(w), 1, K, p(b), None, N, p(y), N, None)
        bi = _lib.BnIn(p(xst), tiles, M, p(gam), p(bet), 1e-5, 0.1, p(rm), p(rv), p(nbt), p(mo), p(io), p(u), p(vo))
        _lib.check(L.fs_linear_f32_ex(gd, bi, p(sto), st()))
        torch.cuda.synchronize()
    finally:
        L.fs_set_lean_gemm(prev)
    ref = torch.relu(torch.nn.functional.batch_norm(xx, None, None, gam, bet, True, 0.1, 1e-5)) @ w.t() + b
    return [y, sto, u, mo, io, vo, rm, rv, nbt], ref, (xx, xst, w, b, gam, bet)


@pytest.mark.parametrize("K", [64, 256])
@pytest.mark.parametrize("M", [512, 480, 256])
def test_full_batch_bn_in_load_product_at_the_pretraining_batch(M, K):
    """gemm_lin_kernel's compile-time full-batch form at 16 row tiles (M = 512, Algorithm 1's
    batch: both rounds of producer statistics as unconditional buffer loads, the Chan combine
    with constant tile sizes) gives the bits of the generic kernels (fs_set_lean_gemm(0)):
    output, a_out, mean, invstd, variance, running statistics and tile statistics.  M = 480
    (15 tiles: the run-time form) and M = 256 (the 8-tile form) are unchanged.  Then a
    512-row and a 256-row problem in one launch (fs_linear_f32_ex2: mixed tile counts take
    the run-time kernel) against each alone."""
    from flowstate import _lib

    N = 64
    lean, ref, _ = _bn_in_load_product(M, K, N, True, M + K)
    generic, _, _ = _bn_in_load_product(M, K, N, False, M + K)
    for i, (a, c) in enumerate(zip(lean, generic)):
        assert torch.equal(a, c), i
    torch.testing.assert_close(lean[0], ref, rtol=1e-4, atol=1e-4)
    assert int(lean[8]) == 1
    if M != 512:
        return
    L, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr
    small, _, _ = _bn_in_load_product(256, K, N, True, M + K)
    ins = [_bn_in_load_product(m, K, N, True, M + K)[2] for m in (512, 256)]
    ys = [torch.empty((m, N), device="cuda") for m in (512, 256)]
    ss = [torch.empty((m // 32, N, 2), device="cuda") for m in (512, 256)]
    gds = [_lib.GemmF32(m, N, K, p(i[0]), K, 1, p(i[2]), 1, K, p(i[3]), None, N, p(y), N, None)
           for m, i, y in zip((512, 256), ins, ys)]
    bis = [_lib.BnIn(p(i[1]), m // 32, m, p(i[4]), p(i[5]), 1e-5, 0.1, None, None, None, None, None, None, None)
           for m, i in zip((512, 256), ins)]
    _lib.check(L.fs_linear_f32_ex2(gds[0], bis[0], p(ss[0]), gds[1], bis[1], p(ss[1]), st()))
    torch.cuda.synchronize()
    assert torch.equal(ys[0], lean[0]) and torch.equal(ss[0], lean[1])
    assert torch.equal(ys[1], small[0]) and torch.equal(ss[1], small[1])
