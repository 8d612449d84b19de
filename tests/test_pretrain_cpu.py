"""Algorithm 1's pretraining stage (flowstate.algorithm1.pretrain, main_algorithm_1.py:268,
294-331) on CPU tensors: the loop against the reference loop written out here, the skip
rule, the output files, and one step on A1's own conditioner against the reference's own
step (tests/golden/pretrain_a1.npz, made by tests/golden/make_pretrain_golden.py).
tests/test_gpu_pretrain.py repeats the step on the MI355X with the checks of this file."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
SMALL = dict(L=2, H=32, nb=1, K=8)


def small_flow(seed=3, device="cpu", **kw):
    """A small flow at N=3 with seeded weights (final layers N(0, 0.05): a non-trivial flow)."""
    from flowstate.models import build_flow
    from oracle import flow as OF

    kw = kw or SMALL
    dims = OF.FlowDims(N=3, B=OF.half_box(3), **kw)
    m = build_flow(3, bound=dims.B, device="cpu", **kw)
    m.load_state_dict(OF.random_state_dict(dims, seed=seed, final_std=0.05), strict=True)
    return m.to(device), dims


def rows(n, B, seed=0):
    return (torch.rand((n, 6), generator=torch.Generator().manual_seed(seed)) * 2 - 1) * B * 0.95


def reference_loop(model, x, epochs, batch_size, lr, wd, drop_row=None):
    """main_algorithm_1.py:268, 294-319 as written.  drop_row: batches that hold that row of
    x never happen (no forward, no step); they are still drawn."""
    from torch.utils.data import DataLoader, TensorDataset

    marked = torch.cat([x, torch.arange(len(x), dtype=x.dtype)[:, None]], 1)
    dataloader = DataLoader(TensorDataset(marked), batch_size=batch_size, shuffle=True)
    loss_hist, loss_epoch = np.array([]), []
    optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd)
    for _ in range(epochs):
        epoch_loss = 0
        for batch in dataloader:
            b = batch[0][:, :-1]
            if drop_row is not None and bool((batch[0][:, -1] == drop_row).any()):
                continue
            optimizer.zero_grad()
            loss = model.forward_kld(b)
            if torch.isnan(loss) or torch.isinf(loss):
                pass
            else:
                loss.backward()
                optimizer.step()
            loss_hist = np.append(loss_hist, loss.to("cpu").data.numpy())
            epoch_loss += loss.item()
        loss_epoch.append(epoch_loss / len(dataloader))
    return loss_hist, loss_epoch, optimizer


def test_pretrain_loop_is_the_reference_loop():
    """40 rows, batch 16 (tail of 8), 3 epochs, graphed=False: the losses, the epoch means
    and every entry of the final state_dict equal the reference loop's under the same seed,
    from (M, N, 2) float64 numpy samples (production's form) as from an (M, 2N) tensor."""
    from flowstate import algorithm1 as A1

    torch.set_num_threads(4)
    m1, dims = small_flow()
    m2, _ = small_flow()
    m3, _ = small_flow()
    x = rows(40, dims.B)
    torch.manual_seed(11)
    want_hist, want_epoch, _ = reference_loop(m1, x, 3, 16, 1e-3, 0.0)
    torch.manual_seed(11)
    got = A1.pretrain(m2, x.double().reshape(40, 3, 2).numpy(), epochs=3, batch_size=16, lr=1e-3, graphed=False)
    assert got.loss_hist.dtype == np.float64 and got.loss_hist.shape == (9,)
    assert np.array_equal(got.loss_hist, want_hist)
    assert got.loss_epoch == want_epoch
    assert got.skipped == 0 and got.adam_steps == 9 and not got.graphed
    assert not m2.training
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    assert list(sd1) == list(sd2)
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
    torch.manual_seed(11)
    again = A1.pretrain(m3, x, epochs=3, batch_size=16, lr=1e-3, graphed=None)  # a CPU model: eager
    assert np.array_equal(again.loss_hist, want_hist) and not again.graphed


def test_pretrain_skips_a_non_finite_loss():
    """A NaN coordinate in one row: the step that draws it records a non-finite loss and is
    skipped; the parameters and Adam's step count are those of a run in which that step never
    happened.  (The BatchNorm running statistics are not compared: the reference's forward
    has updated them, with NaN, before the skip.)"""
    from flowstate import algorithm1 as A1

    torch.set_num_threads(4)
    m1, dims = small_flow()
    m2, _ = small_flow()
    x = rows(40, dims.B)
    bad = x.clone()
    bad[17, 2] = float("nan")
    torch.manual_seed(5)
    want_hist, _, opt = reference_loop(m1, x, 2, 16, 1e-3, 0.0, drop_row=17)
    torch.manual_seed(5)
    got = A1.pretrain(m2, bad, epochs=2, batch_size=16, lr=1e-3, graphed=False)
    assert got.skipped == 2 and got.loss_hist.shape == (6,)
    nonfinite = ~np.isfinite(got.loss_hist)
    assert nonfinite.sum() == 2 and nonfinite[:3].sum() == 1
    assert np.array_equal(got.loss_hist[~nonfinite], want_hist)
    assert all(not np.isfinite(v) for v in got.loss_epoch)  # non-finite losses included (:318-319)
    steps = {int(st["step"]) for st in opt.state.values()}
    assert steps == {4} and got.adam_steps == 4
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p1, p2), n


def test_pretrain_refuses_a_last_batch_of_one_row():
    from flowstate import algorithm1 as A1

    m, dims = small_flow()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        A1.pretrain(m, rows(33, dims.B), epochs=1, batch_size=16, graphed=False)
    with pytest.raises(ValueError, match="samples must be"):
        A1.pretrain(m, rows(32, dims.B)[:, :4], epochs=1, batch_size=16, graphed=False)


def check_pretrain_files(res, model, out_dir, fresh):
    """Both files exist; the JSON holds loss_epoch; the .pth loads with strict=True into the
    fresh model with equal tensors and holds every tensor once (no flat-buffer inflation)."""
    loss_path = os.path.join(out_dir, "loss_function_data.json")
    model_path = os.path.join(out_dir, "initial_model_circularspline_res_dense.pth")
    assert res.files == {"loss": loss_path, "model": model_path}
    with open(loss_path) as f:
        assert json.load(f) == {"loss_epoch": res.loss_epoch}
    sd = torch.load(model_path, map_location="cpu")
    fresh.load_state_dict(sd, strict=True)
    want = model.state_dict()
    assert list(sd) == list(want)
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, want[k].cpu()), k
    payload = sum(v.numel() * v.element_size() for v in want.values())
    assert os.path.getsize(model_path) <= payload + 512 * len(want) + 65536, (os.path.getsize(model_path), payload)


def test_pretrain_writes_the_reference_files(tmp_path):
    from flowstate import algorithm1 as A1

    torch.set_num_threads(4)
    m, dims = small_flow()
    fresh, _ = small_flow(seed=9)
    torch.manual_seed(2)
    res = A1.pretrain(m, rows(40, dims.B), epochs=2, batch_size=16, graphed=False, out_dir=str(tmp_path / "round"))
    assert len(res.loss_epoch) == 2
    check_pretrain_files(res, m, str(tmp_path / "round"), fresh)


# --- one pretraining step on A1's own conditioner (tests/golden/pretrain_a1.npz) -----------
# The checks are those of test_train_cpu.check_a2_step (its reasoning is written out at
# A2_TOL there: each gradient is held to a multiple of the REFERENCE'S OWN float32 error
# against the same step's float64 gradients, Adam's first update to Adam's formula on this
# path's own gradients and, on the whole tensors, to the update on the exact gradients),
# with the same bounds, for Adam(lr=1e-4, weight_decay=0) (main_algorithm_1.py LR /
# WEIGHT_DECAY; both are read from the golden).  Without weight decay the biases in front
# of a train-mode BatchNorm (exactly-zero true gradient, rounding noise of ~1e-9 on both
# sides) move by a noise-sized Adam step; they are covered by check (i) of the update (Adam
# on this path's own gradients) and are not among the golden's whole tensors.
PRETRAIN_TOL = dict(loss_rtol=1e-5, grad_vs_f32_err=1.5, grad_max_vs_f32_err=1.5, grad_abs=1e-7,
                    bn_rtol=1e-4, bn_atol=1e-6, update_vs_f32_err=2.0)


def build_pretrain_a1(device):
    """The golden's flow (A1's conditioner: H=256, 32 blocks, K=32; L=2, N=3) from its seed
    (checksum checked), no target (p = None), train mode."""
    from flowstate.models import build_flow
    from oracle import flow as OF

    f = np.load(os.path.join(G, "pretrain_a1.npz"))
    N, L, H, nb, K = (int(v) for v in f["dims"])
    dims = OF.FlowDims(N=N, L=L, H=H, nb=nb, K=K, B=OF.half_box(N))
    sd = OF.random_state_dict(dims, seed=int(f["seed"]), final_std=0.05)
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    assert h.digest() == f["checksum"].tobytes(), "weights differ from the golden's"
    m = build_flow(N, L=L, H=H, nb=nb, K=K, bound=dims.B, device="cpu")
    m.load_state_dict(sd, strict=True)
    assert m.p is None
    m = m.to(device)
    m.train()
    return m, f


def check_pretrain_step(m, f, loss, grads, before):
    """loss (float), grads {name: tensor or None}, before {name: parameter before the step};
    m holds the parameters and running statistics after the step.  Returns the measured
    multiples (whole-tensor gradient 2-norm, max-abs, per-tensor norm, update)."""
    t = PRETRAIN_TOL
    lr, wd = float(f["lr"]), float(f["wd"])
    np.testing.assert_allclose(loss, float(f["step_loss"]), rtol=t["loss_rtol"])
    names = [str(n) for n in f["names"]]
    params = dict(m.named_parameters())
    assert names == list(params)
    worst = worst_n = worst_mx = 0.0
    for n, gn, e32 in zip(names, f["grad_norm"], f["grad_err32_norm"]):
        g = grads.get(n)
        if gn < 0:  # no gradient in the reference (unused preprocessing weights)
            assert g is None or not g.abs().max().item(), n
            continue
        d32 = abs(float(g.double().norm()) - gn)
        assert d32 <= t["grad_vs_f32_err"] * e32 + t["grad_abs"], (n, d32, e32)
        if e32 > t["grad_abs"]:
            worst_n = max(worst_n, d32 / e32)
        if "grad/" + n in f:
            g64 = torch.from_numpy(f["grad64/" + n]).double()
            ref32 = torch.from_numpy(f["grad/" + n]).double()
            gg = g.double().cpu()
            e, e_ref = float((gg - g64).norm()), float((ref32 - g64).norm())
            mx, mx_ref = float((gg - g64).abs().max()), float((ref32 - g64).abs().max())
            print(f"  grad {n}: |g - g64| = {e:.3e} (reference's float32: {e_ref:.3e}), max-abs {mx:.3e} ({mx_ref:.3e}), "
                  f"|g64| = {float(g64.norm()):.3e}")
            assert e <= t["grad_vs_f32_err"] * e_ref + t["grad_abs"], (n, e, e_ref)
            assert mx <= t["grad_max_vs_f32_err"] * mx_ref + t["grad_abs"], (n, mx, mx_ref)
            if e_ref > t["grad_abs"]:
                worst = max(worst, e / e_ref)
                worst_mx = max(worst_mx, mx / mx_ref)
    print(f"A1 pretraining step: worst whole-tensor gradient error vs float64 = {worst:.2f} x the reference's "
          f"float32 error (max-abs {worst_mx:.2f} x; per-tensor norm {worst_n:.2f} x)")
    seen = 0
    for k, v in m.state_dict().items():
        if "bn/" + k in f:
            ref = f["bn/" + k]
            seen += 1
            if "num_batches" in k:
                assert int(v) == int(ref), k
            else:
                np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=t["bn_rtol"], atol=t["bn_atol"], err_msg=k)
    assert seen == sum(k.startswith("bn/") for k in f.files)

    def adam_first(g, p0):  # torch.optim.Adam's first step (L2 weight decay), float64
        gp = g.double() + wd * p0.double()
        return -lr * gp / (gp.abs() + 1e-8)

    worst_u = 0.0
    for n, gn in zip(names, f["grad_norm"]):
        p0, p1 = before[n], params[n].detach()
        d = (p1 - p0).double()
        if gn < 0:
            assert not d.abs().max().item(), n  # no gradient: Adam leaves it alone
            continue
        want = adam_first(grads[n], p0)
        # torch's Adam runs in float32 with beta2 = 0.999 rounded to float (its bias
        # correction 1 - 0.999f is 1.3e-5 off 0.001): updates agree with the exact formula
        # to ~1e-5 relative, plus the rounding of p itself
        ulp = 2.0 ** -23 * torch.maximum(p0.abs(), p1.abs()).double()
        assert bool(((d - want).abs() <= 2 * ulp + 5e-5 * want.abs() + 1e-6 * lr).all()), \
            (n, float((d - want).abs().max()))
        if "update/" + n in f:
            g64 = torch.from_numpy(f["grad64/" + n]).to(p0.device)
            d64 = adam_first(g64, p0)
            ref = torch.from_numpy(f["update/" + n]).double().to(d.device)
            e, e_ref = float((d - d64).norm()), float((ref - d64).norm())
            print(f"  update {n}: |d - d64| = {e:.3e} (reference's float32: {e_ref:.3e}), |d64| = {float(d64.norm()):.3e}")
            assert e <= t["update_vs_f32_err"] * e_ref + 1e-7, (n, e, e_ref)
            if e > 1e-7:  # above the absolute floor
                worst_u = max(worst_u, e / max(e_ref, 1e-30))
    print(f"A1 pretraining step: worst whole-tensor Adam update error vs float64 (above 1e-7) = {worst_u:.2f} x "
          f"the reference's")
    return worst, worst_mx, worst_n, worst_u


def test_pretraining_step_matches_reference_on_a1_conditioner_cpu():
    """One forward_kld / Adam step at batch 512 on A1's conditioner through the host-side
    torch restatement (CPU tensors) against the reference's own step."""
    torch.set_num_threads(8)
    m, f = build_pretrain_a1("cpu")
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    x = torch.from_numpy(f["x"])
    assert x.shape == (512, 6)
    opt = torch.optim.Adam(m.parameters(), lr=float(f["lr"]), weight_decay=float(f["wd"]))
    opt.zero_grad()
    loss = m.forward_kld(x)
    loss.backward()
    grads = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()}
    opt.step()
    check_pretrain_step(m, f, loss.item(), grads, before)
