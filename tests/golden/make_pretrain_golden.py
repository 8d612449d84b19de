"""Generate tests/golden/pretrain_a1.npz by running the REFERENCE itself.

Container-only, like make_goldens.py (whose import recipe it uses): the reference is
imported read-only and only arrays are stored.  Re-run with

    python tests/golden/make_pretrain_golden.py

pretrain_a1.npz: one step of the Algorithm-1 pretraining loop (main_algorithm_1.py:297-314)
on A1's own conditioner: a flow of L=2 layers with H=256, 32 residual blocks and K=32 bins
at N=3 (two layers are the smallest depth with an inter-layer backward hand-off; the
driver's 15 repeat them) in train mode, seeded weights (oracle.flow.random_state_dict,
seed 47, final layers N(0, 0.05); only the seed and the checksum are stored), a fresh
Adam(lr=1e-4, weight_decay=0), one batch of 512 training rows, loss = forward_kld(batch)
alone.  Stored, as train_a2.npz does for the Algorithm-2 step (make_goldens.train_a2_case,
which this mirrors with the sampling pass removed): the float32 loss, every parameter
gradient's norm, the same step's gradients by the reference model in float64 as the exact
values (|g32 - g64| per tensor), a few small tensors whole (gradient, float64 gradient,
Adam update), every update's norm, and the BatchNorm running statistics after the step.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "flow-state_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_goldens import build_ref_model, import_reference, sd_checksum  # noqa: E402

N, L, H, NB, K, BATCH, SEED = 3, 2, 256, 32, 32, 512, 47
LR, WD = 1e-4, 0.0  # main_algorithm_1.py LR / WEIGHT_DECAY

# the tensors stored whole: small ones only (biases, BatchNorm weights, the 256 x 6 initial weight)
PRETRAIN_FULL = ("flows.0.prqct.transform_net.initial_layer.weight",
                 "flows.0.prqct.transform_net.initial_layer.bias",
                 "flows.0.prqct.transform_net.blocks.15.batch_norm_layers.0.bias",
                 "flows.0.prqct.transform_net.blocks.31.linear_layers.1.bias",
                 "flows.0.prqct.transform_net.final_layer.bias",
                 "flows.1.prqct.transform_net.initial_layer.weight",
                 "flows.1.prqct.transform_net.blocks.0.batch_norm_layers.1.weight",
                 "flows.1.prqct.transform_net.blocks.16.batch_norm_layers.0.weight",
                 "flows.1.prqct.transform_net.final_layer.bias")


def training_rows(dims):
    """512 rows as the driver feeds them (box configurations - HALF_BOX): half the left-well
    start of the even runs (initialise_low_left) with thermal jitter, wrapped into the box,
    half uniform in 0.95 B."""
    from flowstate.MCMC.initialise import initialise_low_left

    rng = np.random.default_rng(SEED + 2)
    B = dims.B
    low, _ = initialise_low_left(num_particles=N, rho=0.03, aspect_ratio=1.0)
    lat = low[None] + rng.normal(0, 0.35, (BATCH // 2, N, 2))
    lat = np.mod(lat, 2 * B) - B
    uni = (rng.random((BATCH - BATCH // 2, N, 2)) * 2 - 1) * B * 0.95
    return torch.from_numpy(np.concatenate([lat, uni]).reshape(BATCH, -1).astype(np.float32))


def pretrain_case(NF):
    from oracle import flow as OF

    dims = OF.FlowDims(N=N, L=L, H=H, nb=NB, K=K, B=OF.half_box(N))
    sd = OF.random_state_dict(dims, seed=SEED, final_std=0.05)
    x = training_rows(dims)
    real_zeros = torch.zeros

    def zeros_cpu(*a, **k):
        if k.get("device") == "cuda":
            k["device"] = "cpu"
        return real_zeros(*a, **k)

    model = build_ref_model(NF, dims)
    model.load_state_dict(sd, strict=True)
    model.train()
    names = [n for n, _ in model.named_parameters()]
    assert all(n in names for n in PRETRAIN_FULL)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    out = {"x": x.numpy(), "seed": np.int64(SEED), "names": np.array(names), "lr": np.float64(LR),
           "wd": np.float64(WD), "dims": np.array([N, L, H, NB, K], dtype=np.int64),
           "checksum": np.frombuffer(bytes.fromhex(sd_checksum(sd)), dtype=np.uint8)}
    torch.zeros = zeros_cpu
    try:
        opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD)
        opt.zero_grad()
        loss = model.forward_kld(x)
        out["fkld"] = loss.detach().numpy()
        out["step_loss"] = loss.detach().numpy()
        assert not (torch.isnan(loss) or torch.isinf(loss))
        loss.backward()
        gnorm, dnorm = [], []
        for n, p in model.named_parameters():
            g = p.grad
            gnorm.append(float(g.double().norm()) if g is not None else -1.0)
            if n in PRETRAIN_FULL:
                out["grad/" + n] = g.numpy().copy()
        opt.step()
        for n, p in model.named_parameters():
            d = p.detach() - before[n]
            dnorm.append(float(d.double().norm()))
            if n in PRETRAIN_FULL:
                out["update/" + n] = d.numpy()
        out["grad_norm"] = np.array(gnorm)
        out["update_norm"] = np.array(dnorm)
        for k, v in model.state_dict().items():
            if "running" in k or "num_batches" in k:
                out["bn/" + k] = v.numpy()
        # the reference's own float32 error: the same step's gradients in float64
        g32 = {n: p.grad.detach().double().clone() for n, p in model.named_parameters() if p.grad is not None}
        m64 = build_ref_model(NF, dims)
        m64.load_state_dict(sd, strict=True)
        m64 = m64.double()
        m64.train()
        l64 = m64.forward_kld(x.double())
        l64.backward()
        err = []
        for n, p in m64.named_parameters():
            if n in g32:
                err.append(float((g32[n] - p.grad.detach()).norm()))
                if n in PRETRAIN_FULL:
                    out["grad64/" + n] = p.grad.detach().numpy().copy()
            else:
                err.append(-1.0)
        out["grad_err32_norm"] = np.array(err)
        out["fkld64"] = l64.detach().numpy()
    finally:
        torch.zeros = real_zeros
    path = os.path.join(HERE, "pretrain_a1.npz")
    np.savez_compressed(path, **out)
    print("pretrain_a1: ok", float(out["fkld"]), float(out["fkld64"]), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    NF, _, _ = import_reference()
    pretrain_case(NF)
