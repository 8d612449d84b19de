"""Graphed training steps/s of the general-shape mode at an uninstantiated bin count, and the
runtime-K coupling kernels against the instantiated ones at a bin count both cover.

One step = train.GraphedTrainStep (reverse_kld's sampling pass + forward_kld + backward +
Adam, ALPHA = 1), batch 256, N = 64, synthetic training configurations (FCC + jitter) as
tools/bench_train.py.  Cases:
  a  L=23 H=96 nb=2 K=10 in "f32-general" (no kernel is instantiated for K = 10);
  b  the A2 flow (L=23 H=128 nb=2 K=15) in the default mode: instantiated coupling kernels;
  c  the A2 flow with autograd_flow._force_any_k: the same step on the runtime-K kernels.
Every case is captured once; then rounds of `--steps` replays alternate between the cases,
timed with device events; the figure is the median round.  A case whose step cannot be
captured is timed eagerly instead and marked "graphed": false.  The timings are printed as one
JSON line; then the launches per step are counted and the line is printed again with them:
the device kernels the profiler records in the step's loss + backward run eagerly (the
launches the graph holds, without Adam's one), all of them and those of the conditioner GEMMs
and coupling layers (the count tests/test_gpu_paired.py pins).  No replay runs under the
profiler."""
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

N, BATCH = 64, 256
LR, WD = 0.000543510751759681, 9.5857178422352e-05
CASES = {"a": (dict(L=23, H=96, nb=2, K=10), "f32-general", False),
         "b": (A2, "f32", False),
         "c": (A2, "f32", True)}


class _Eager:
    """The step outside a graph, for a tree that cannot capture it."""

    def __init__(self, m):
        self.m = m
        self.opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)

    def step(self, x):
        self.opt.zero_grad()
        loss = step_loss(self.m, x, BATCH, 1.0)
        loss.backward()
        self.opt.step()
        return loss


def build(case, data):
    kw, mode, force = CASES[case]
    torch.manual_seed(0)
    B = half_box(N)
    m = build_flow(N, bound=B, device="cpu", **kw)
    m.p = DoubleWellLJ(2 * N, N, 1.0, B, V0_list=[-10.0, -10.5], r0=1.2, k=15)
    m = m.cuda().set_precision(mode).train()
    m.q0.device = torch.device("cuda")
    AF._force_any_k = force  # read when the step's launches are recorded
    try:
        try:
            g = GraphedTrainStep(m, BATCH, lr=LR, weight_decay=WD, alpha=1.0, example=data[:BATCH])
            return g, True, bool(g.flat_bn is not None and AF._last_paired)
        except Exception as e:  # noqa: BLE001 (reported in the result)
            sys.stderr.write(f"case {case}: capture failed ({type(e).__name__}: {e}); timing the eager step\n")
            torch.cuda.synchronize()
            m.train()
            return _Eager(m), False, False
    finally:
        AF._force_any_k = False


def launches(g, x):
    """Device kernels of one eager loss + backward of the step g holds."""
    from torch.profiler import ProfilerActivity, profile

    m = g.model if isinstance(g, GraphedTrainStep) else g.m
    flat_bn = g.flat_bn if isinstance(g, GraphedTrainStep) else None
    for p in m.parameters():
        p.grad = None
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        loss = step_loss(m, x, BATCH, 1.0, flat_bn)
        loss.backward()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]
    return len(kernels), sum(1 for n in kernels if "gemm" in n or "coupling" in n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-launches", action="store_true", help="timings only: skip the launch count")
    a = ap.parse_args()
    cases = a.cases.split(",")
    B = half_box(N)
    base, _ = initialise_fcc(num_particles=N, rho=0.03, aspect_ratio=1.0)
    rng = np.random.default_rng(3)
    data = np.mod(base[None] + rng.normal(0, 0.3, (BATCH * 8, N, 2)), 2 * B) - B
    data = torch.from_numpy(data.astype(np.float32).reshape(-1, 2 * N)).cuda()
    xb = [data[i * BATCH:(i + 1) * BATCH] for i in range(8)]
    steps, res = {}, {}
    for c in cases:
        g, graphed, paired = build(c, data)
        steps[c] = g
        for i in range(a.warmup):
            g.step(xb[i % 8])
        torch.cuda.synchronize()
        res[c] = {"graphed": graphed, "paired": paired, "shape": dict(CASES[c][0]), "mode": CASES[c][1],
                  "force_any_k": CASES[c][2], "round_ms": []}
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
        ms = statistics.median(res[c]["round_ms"])
        res[c].update(ms_per_step=ms, steps_per_s=1e3 / ms, round_ms=[round(v, 4) for v in res[c]["round_ms"]])
    out = {"metric": "graphed training steps/s, batch 256, N=64, ALPHA=1 (median of alternating rounds, device events)",
           "rounds": a.rounds, "steps_per_round": a.steps, "cases": res}
    if "b" in res and "c" in res:
        out["runtime_k_over_instantiated"] = res["c"]["steps_per_s"] / res["b"]["steps_per_s"]
    print(json.dumps(out), flush=True)
    if a.no_launches:
        return
    for c in cases:
        AF._force_any_k = CASES[c][2]
        try:
            n, nlayer = launches(steps[c], xb[0])
        finally:
            AF._force_any_k = False
        res[c].update(launches_per_step=n, gemm_and_coupling_launches_per_step=nlayer)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
