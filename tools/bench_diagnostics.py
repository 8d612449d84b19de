"""Timings of the chain diagnostics on the device, by device events in one process (timing
only; nothing imports this): one fs_chain_observe launch, then fs_chain_autocov (W = 256),
fs_chain_tau, fs_chain_pool and fs_chain_transitions on a [T][C] series, at the benchmark's
scale (C = 65,536, T = 1000, N = 64) and at the Algorithm-1 regime's (C = 10, T = 1000,
N = 3).  Beside the autocovariance, as the only yardstick, a float64 torch statement of the
same lag sums on the device, `(d[:T-k] * d[k:]).sum(0)` per lag.  Warm-up first, then the
median of 5 rounds with min and max.  Prints one JSON line (and writes it to --out)."""
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

from flowstate import _lib, diagnostics  # noqa: E402
from flowstate.MCMC import BatchedMonteCarlo, Physics  # noqa: E402


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def timed(fn, iters, rounds):
    assert fn() in (0, None)
    window(fn, max(1, iters // 4))  # warm-up
    ts = [window(fn, iters) for _ in range(rounds)]
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), rounds=rounds, iters=iters)


def torch_lag_sums(x, W):
    T = x.shape[0]
    d = x - x.mean(0)
    out = torch.empty((W + 1, x.shape[1]), dtype=torch.float64, device=x.device)
    for k in range(W + 1):
        out[k] = (d[:T - k] * d[k:]).sum(0) / T
    return out


def scale(C, T, N, W, rounds, heavy_iters):
    dev = torch.device("cuda", torch.cuda.current_device())
    L, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
    rng = np.random.default_rng(0)
    box = float(np.sqrt(N / 0.03))
    centres = np.array([[box / 4, box / 2], [3 * box / 4, box / 2]])
    state = centres[rng.integers(0, 2, (C, 1))] + rng.uniform(-1.0, 1.0, (C, N, 2))
    bmc = BatchedMonteCarlo(None, state, Physics(box, box), np.arange(1, C + 1, dtype=np.uint64), device=dev)
    bmc.state_is_f32.copy_(torch.arange(C, device=dev) % 2)
    rec = diagnostics.ChainRecorder(bmc, 2)
    res = {"C": C, "T": T, "N": N, "W": W}
    res["fs_chain_observe"] = timed(lambda: (rec.reset(), rec.record())[1], 200, rounds)
    del rec
    # an AR(1) series per chain (phi = 0.9) and well counts that hop now and then
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.empty((T, C), dtype=torch.float64, device=dev)
    x[0] = torch.randn(C, generator=g, device=dev, dtype=torch.float64)
    for t in range(1, T):
        x[t] = 0.9 * x[t - 1] + torch.randn(C, generator=g, device=dev, dtype=torch.float64)
    well = (torch.rand((T, C), generator=g, device=dev) < 0.5)
    n_a = torch.where(well, N, 0).to(torch.uint8)
    n_b = torch.where(well, 0, N).to(torch.uint8)
    mean = torch.empty(C, dtype=torch.float64, device=dev)
    acov = torch.empty((W + 1, C), dtype=torch.float64, device=dev)
    tau = torch.empty(C, dtype=torch.float64, device=dev)
    win = torch.empty(C, dtype=torch.int32, device=dev)
    flags = torch.empty(C, dtype=torch.uint8, device=dev)
    pooled = torch.empty(W + 1, dtype=torch.float64, device=dev)
    scalars = torch.empty(4, dtype=torch.float64, device=dev)
    table = torch.empty((C, 6), dtype=torch.int64, device=dev)
    res[f"fs_chain_autocov (f64, W={W})"] = timed(
        lambda: L.fs_chain_autocov(p(x), 0, T, C, C, W, p(mean), p(acov), st), heavy_iters, rounds)
    res[f"fs_chain_autocov (u8, W={W})"] = timed(
        lambda: L.fs_chain_autocov(p(n_a), 1, T, C, C, W, p(mean), p(acov), st), heavy_iters, rounds)
    L.fs_chain_autocov(p(x), 0, T, C, C, W, p(mean), p(acov), st)
    res["fs_chain_tau"] = timed(lambda: L.fs_chain_tau(p(mean), p(acov), C, W, 5.0, p(tau), p(win), p(flags), st),
                                50, rounds)
    res["fs_chain_pool"] = timed(lambda: L.fs_chain_pool(p(mean), p(acov), C, W, T, p(pooled), p(scalars), st),
                                 50, rounds)
    res["fs_chain_transitions"] = timed(lambda: L.fs_chain_transitions(p(n_a), p(n_b), T, C, C, N, p(table), st),
                                        50, rounds)
    ref = torch_lag_sums(x, W)
    res["max_rel_diff_vs_torch"] = float(((acov - ref).abs().max() / ref.abs().max()).item())
    res[f"torch lag sums (f64, W={W})"] = timed(lambda: (torch_lag_sums(x, W), None)[1], max(1, heavy_iters // 5),
                                                rounds)
    res["tau_median"] = float(tau.median().item())
    res["flags_nonzero"] = int((flags != 0).sum().item())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-lag", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with _lib.on_device(torch.device("cuda", torch.cuda.current_device())):
        res = {"benchmark scale": scale(65536, 1000, 64, args.max_lag, args.rounds, 10),
               "algorithm-1 regime": scale(10, 1000, 3, args.max_lag, args.rounds, 50)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
