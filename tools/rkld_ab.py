"""Graphed training steps/s at ALPHA = 0.5 (the sampling pass differentiable) with the fused
sampling-pass backward (autograd_flow._fused_sample_grad, the default) against the per-op
coupling path it replaces (the switch off: coupling_sample over torch ops and the element-wise
spline kernels, the loss head in torch), in one process.

One step = train.GraphedTrainStep (reverse_kld + forward_kld + backward + Adam, ALPHA = 0.5),
batch 256, N = 64, synthetic training configurations (FCC + jitter) as tools/bench_train.py.
Shapes:
  a2       the A2 flow (L=23 H=128 nb=2 K=15), default mode: instantiated coupling kernels;
  general  L=23 H=96 nb=2 K=10 in "f32-general": the runtime-K coupling kernels.
Each (shape, switch) pair is captured once, the switch set while it is captured; then rounds of
`--steps` replays alternate between the four graphs, timed with device events; the figure is
the median round and "spread" is (max - min) / median over the rounds.  The timings are printed
as one JSON line; then the launches per step are counted and the line is printed again with
them: the device kernels the profiler records in the step's loss + backward run eagerly (the
launches the graph holds, without Adam's one).  No replay runs under the profiler."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "flow-state_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from flowstate.MCMC import initialise_fcc  # noqa: E402
from flowstate.models import A2, build_flow, half_box  # noqa: E402
from flowstate.normflows import autograd_flow as AF  # noqa: E402
from flowstate.normflows.Energy import DoubleWellLJ  # noqa: E402
from flowstate.normflows.train import GraphedTrainStep, step_loss  # noqa: E402

N, BATCH, ALPHA = 64, 256, 0.5
LR, WD = 0.000543510751759681, 9.5857178422352e-05
SHAPES = {"a2": (A2, "f32"), "general": (dict(L=23, H=96, nb=2, K=10), "f32-general")}


def build(shape, fused, data):
    kw, mode = SHAPES[shape]
    torch.manual_seed(0)
    B = half_box(N)
    m = build_flow(N, bound=B, device="cpu", **kw)
    m.p = DoubleWellLJ(2 * N, N, 1.0, B, V0_list=[-10.0, -10.5], r0=1.2, k=15)
    m = m.cuda().set_precision(mode).train()
    m.q0.device = torch.device("cuda")
    prev = AF._fused_sample_grad
    AF._fused_sample_grad = fused  # read when the step's launches are recorded
    try:
        n0 = AF.sample_grad_steps
        g = GraphedTrainStep(m, BATCH, lr=LR, weight_decay=WD, alpha=ALPHA, example=data[:BATCH])
        assert (AF.sample_grad_steps > n0) == fused
        return g
    finally:
        AF._fused_sample_grad = prev


def launches(g, fused, x):
    """Device kernels of one eager loss + backward of the step g holds."""
    from torch.profiler import ProfilerActivity, profile

    prev = AF._fused_sample_grad
    AF._fused_sample_grad = fused
    try:
        for p in g.model.parameters():
            p.grad = None
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            loss = step_loss(g.model, x, BATCH, ALPHA, g.flat_bn)
            loss.backward()
            torch.cuda.synchronize()
    finally:
        AF._fused_sample_grad = prev
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]
    return len(kernels), sum(1 for n in kernels if "gemm" in n or "coupling" in n or "rqs_" in n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a2,general")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    B = half_box(N)
    base, _ = initialise_fcc(num_particles=N, rho=0.03, aspect_ratio=1.0)
    rng = np.random.default_rng(3)
    data = np.mod(base[None] + rng.normal(0, 0.3, (BATCH * 8, N, 2)), 2 * B) - B
    data = torch.from_numpy(data.astype(np.float32).reshape(-1, 2 * N)).cuda()
    xb = [data[i * BATCH:(i + 1) * BATCH] for i in range(8)]
    cases = [(s, f) for s in a.shapes.split(",") for f in (False, True)]
    steps, res = {}, {}
    for c in cases:
        g = steps[c] = build(c[0], c[1], data)
        for i in range(a.warmup):
            g.step(xb[i % 8])
        torch.cuda.synchronize()
        res[c] = {"shape": dict(SHAPES[c[0]][0]), "mode": SHAPES[c[0]][1], "fused_sample_grad": c[1], "round_ms": []}
    for r in range(a.rounds):
        for c in (cases if r % 2 == 0 else cases[::-1]):
            g = steps[c]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.steps):
                loss = g.step(xb[i % 8])
            e1.record()
            e1.synchronize()
            assert bool(torch.isfinite(loss)), c
            res[c]["round_ms"].append(e0.elapsed_time(e1) / a.steps)
    for c in cases:
        rounds = res[c]["round_ms"]
        ms = statistics.median(rounds)
        res[c].update(ms_per_step=ms, steps_per_s=1e3 / ms, spread=(max(rounds) - min(rounds)) / ms,
                      round_ms=[round(v, 4) for v in rounds])
    out = {"metric": "graphed training steps/s, batch 256, N=64, ALPHA=0.5 (median of alternating rounds, device events)",
           "rounds": a.rounds, "steps_per_round": a.steps,
           "cases": {f"{s}/{'fused' if f else 'per-op'}": res[(s, f)] for s, f in cases}}
    for s in a.shapes.split(","):
        out[f"{s}_fused_over_per_op"] = res[(s, True)]["steps_per_s"] / res[(s, False)]["steps_per_s"]
    print(json.dumps(out), flush=True)
    for c in cases:
        n, nlayer = launches(steps[c], c[1], xb[0])
        res[c].update(launches_per_step=n, gemm_coupling_and_spline_launches_per_step=nlayer)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
