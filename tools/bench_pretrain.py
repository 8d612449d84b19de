"""Algorithm-1 pretraining throughput (main_algorithm_1.py:297-319) at the driver's own size:
the A1 flow (L=15, H=256, 32 residual blocks, K=32) at N=3, batch 512, forward_kld only,
Adam(lr=1e-4, weight_decay=0); weights from oracle.flow.random_state_dict, training rows
generated here (left- / right-well starts with jitter, centred).  Prints the result as one JSON
line after the graphed timing and again, complete, at the end:

  * graphed steps/s: GraphedTrainStep(..., reverse=False) replays as pretrain() issues them
    (back to back, check=False), device events around `--steps` replays, the median of
    `--rounds` rounds with their spread;
  * eager steps/s: the reference loop's step (model.forward_kld, backward, torch.optim.Adam,
    the host-side skip test) on a second model, device events around `--steps` steps;
  * device kernels per step (torch profiler around one eager loss + backward, plus Adam's
    one launch and the graph's running-statistics snapshot / restore), and, when the
    profiler reports them, the kernels of one graph replay;
  * the MFMA floor of a step from the shapes (forward products x 3 over the float32
    matrix rate) and the graphed step's fraction of it;
  * the full run (epochs x batches dependent steps) extrapolated from the graphed rate: it
    is not run;
  * --cpu-steps K: the package's CPU step (pretrain(graphed=False) on a CPU model) on
    --cpu-threads host threads, for context;
  * --ab-lib PATH: the same graphed step captured a second time through another build of
    libflowstate.so (tools/build_variant.sh) on a third model, the two replayed in
    alternating rounds in this process: medians, spreads and whether the difference
    exceeds the round-to-round spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "flow-state_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from flowstate import _lib  # noqa: E402
from flowstate import algorithm1 as A1  # noqa: E402
from flowstate.MCMC.initialise import initialise_low_left, initialise_low_right  # noqa: E402
from flowstate.models import A1 as A1_SHAPE, build_flow, half_box  # noqa: E402
from oracle import flow as OF  # noqa: E402

N, BATCH, LR, WD = 3, 512, 1e-4, 0.0
EPOCHS, SAMPLES = 100, 102400  # main_algorithm_1.py:56-66
PEAK_F32_MATRIX = 157.3e12  # FLOP/s, MI355X float32 MFMA


def training_rows(n, B, seed=3):
    rng = np.random.default_rng(seed)
    left, _ = initialise_low_left(num_particles=N, rho=0.03, aspect_ratio=1.0)
    right, _ = initialise_low_right(num_particles=N, rho=0.03, aspect_ratio=1.0)
    base = np.where((np.arange(n) % 2 == 0)[:, None, None], left[None], right[None])
    x = np.mod(base + rng.normal(0, 0.35, (n, N, 2)), 2 * B) - B
    return torch.from_numpy(x.reshape(n, -1).astype(np.float32))


def step_flops(shape, batch):
    """FLOP of one step's matrix products: per row and layer 2 (in H + 2 nb H^2 + H out)
    forward, and twice that backward (input and weight gradients)."""
    D = 2 * N
    n_id = D // 2
    n_tr = D - n_id
    fin, fout = 2 * n_id, n_tr * (3 * shape["K"] + 1)
    H, nb = shape["H"], shape["nb"]
    fwd = 2 * (fin * H + 2 * nb * H * H + H * fout)
    return 3 * fwd * shape["L"] * batch


def model_on(device, sd, shape, B):
    m = build_flow(N, bound=B, device="cpu", **shape)
    m.load_state_dict(sd, strict=True)
    return m.to(device).train()


def timed_rounds(fns, rounds, steps):
    """Each fn in alternating order per round; ms per step from device events."""
    out = [[] for _ in fns]
    for r in range(rounds):
        order = range(len(fns)) if r % 2 == 0 else range(len(fns) - 1, -1, -1)
        for i in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for s in range(steps):
                fns[i](s)
            e1.record()
            e1.synchronize()
            out[i].append(e0.elapsed_time(e1) / steps)
    return out


def summary(ms):
    med = statistics.median(ms)
    return {"ms_per_step": med, "steps_per_s": 1e3 / med, "round_ms": [round(v, 4) for v in ms],
            "spread_ms": max(ms) - min(ms)}


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len([n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=A1_SHAPE["L"])
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=0)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--ab-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pretrain needs the MI355X: nothing is measured without it")
    from flowstate.normflows.train import GraphedTrainStep, step_loss

    shape = dict(A1_SHAPE, L=a.layers)
    B = half_box(N)
    dims = OF.FlowDims(N=N, B=B, **shape)
    sd = OF.random_state_dict(dims, seed=1, final_std=0.05)
    rows = training_rows(8 * BATCH, B)
    data = rows.cuda()
    xb = [data[i * BATCH:(i + 1) * BATCH] for i in range(8)]
    floor_ms = step_flops(shape, BATCH) / PEAK_F32_MATRIX * 1e3
    out = {"metric": "Algorithm-1 pretraining steps/s (forward_kld + Adam, HIP-graph step; device events, median of rounds)",
           "config": {"workload": f"A1: L={shape['L']} H={shape['H']} blocks={shape['nb']} K={shape['K']}, N={N}, "
                                  f"batch {BATCH}, lr {LR}, wd {WD}"},
           "lib": os.environ.get("FLOWSTATE_LIB") or "in-tree", "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "step_gflop": step_flops(shape, BATCH) / 1e9, "mfma_floor_ms": floor_ms}

    m = model_on("cuda", sd, shape, B)
    g = GraphedTrainStep(m, BATCH, LR, WD, example=xb[0], reverse=False)
    steps = [g]
    labels = ["graphed"]
    if a.ab_lib:
        base = _lib.load()
        other = _lib.load(os.path.abspath(a.ab_lib))
        m_ab = model_on("cuda", sd, shape, B)
        _lib._lib = other  # the capture below records the other build's kernels
        try:
            steps.append(GraphedTrainStep(m_ab, BATCH, LR, WD, example=xb[0], reverse=False))
        finally:
            _lib._lib = base
        labels.append("graphed_ab_lib")
    fns = [(lambda s, g=g_: g.step(xb[s % 8], check=False)) for g_ in steps]
    for g_ in steps:
        g_.reset_nan()
    for f in fns:
        for s in range(a.warmup):
            f(s)
    torch.cuda.synchronize()
    ms = timed_rounds(fns, a.rounds, a.steps)
    assert not any(bool(g_.nan_state()) for g_ in steps)
    for lab, v, g_ in zip(labels, ms, steps):
        out[lab] = summary(v)
        out[lab]["last_loss"] = float(g_.graphs[BATCH].loss)
    out["value"], out["unit"] = out["graphed"]["steps_per_s"], "steps/s"
    out["fraction_of_mfma_floor"] = floor_ms / out["graphed"]["ms_per_step"]
    n_steps = EPOCHS * (SAMPLES // BATCH)
    out["full_run_extrapolated"] = {"steps": n_steps, "seconds": n_steps * out["graphed"]["ms_per_step"] / 1e3,
                                    "note": "extrapolated from the graphed rate, not run"}
    if a.ab_lib:
        d = out["graphed_ab_lib"]["ms_per_step"] - out["graphed"]["ms_per_step"]
        spread = max(out["graphed"]["spread_ms"], out["graphed_ab_lib"]["spread_ms"])
        out["ab"] = {"ab_lib": a.ab_lib, "ab_lib_minus_lib_ms": d, "round_spread_ms": spread,
                     "lib_faster_beyond_spread": bool(d > spread),
                     "params_bit_identical": all(torch.equal(p, q) for p, q in
                                                 zip(m.state_dict().values(), m_ab.state_dict().values()))}
    print(json.dumps(out), flush=True)

    # kernels per step: one eager loss + backward of the graph's own step under the profiler
    def fwd_bwd():
        for p in m.parameters():
            p.grad = None
        step_loss(m, xb[0], BATCH, 1.0, g.flat_bn, reverse=False).backward()

    fwd_bwd()
    n_fb = count_kernels(fwd_bwd)
    out["kernels_loss_and_backward"] = n_fb
    # + Adam's launch, the snapshot copies and the restore's selects (its few condition kernels not counted)
    out["kernel_nodes_per_step"] = n_fb + 1 + 2 * len(g.graphs[BATCH].keep)
    try:
        n_replay = count_kernels(lambda: g.step(xb[0], check=False))
        if n_replay:
            out["kernels_in_one_replay_profiled"] = n_replay
    except Exception as e:  # noqa: BLE001 (reported)
        out["replay_profile_error"] = f"{type(e).__name__}: {e}"

    if not a.no_eager:
        me = model_on("cuda", sd, shape, B)
        opt = torch.optim.Adam(me.parameters(), lr=LR, weight_decay=WD)

        def eager(s):
            opt.zero_grad()
            loss = me.forward_kld(xb[s % 8])
            if torch.isnan(loss) or torch.isinf(loss):
                return
            loss.backward()
            opt.step()

        for s in range(min(a.warmup, 5)):
            eager(s)
        torch.cuda.synchronize()
        out["eager"] = summary(timed_rounds([eager], 1, a.steps)[0])
        out["graphed_over_eager"] = out["eager"]["ms_per_step"] / out["graphed"]["ms_per_step"]

    if a.cpu_steps > 0:
        torch.set_num_threads(a.cpu_threads)
        mc = model_on("cpu", sd, shape, B)
        A1.pretrain(mc, rows[:BATCH], epochs=1, batch_size=BATCH, lr=LR, weight_decay=WD, graphed=False)  # warm-up
        t0 = time.perf_counter()
        A1.pretrain(mc, rows[:BATCH * a.cpu_steps], epochs=1, batch_size=BATCH, lr=LR, weight_decay=WD, graphed=False)
        dt = (time.perf_counter() - t0) / a.cpu_steps
        out["cpu_step"] = {"ms_per_step": dt * 1e3, "steps_per_s": 1 / dt, "threads": a.cpu_threads,
                           "steps": a.cpu_steps, "clock": "host"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
