"""Timings of the importance-weighted analysis batch on the device, by device events
(timing only; nothing imports this):

  batch       analysis.sample_analysis on the A2 flow (L=23, H=128, 2 blocks, K=15), N = 64,
              50,000 samples in batches of 1000, results copied to the host at the end, three
              ways in alternation: reweight=None (the batch as it was), reweight set (log q of
              the sampling pass), reweight with density_pass=True (one more flow pass per batch)
  kernels     ms per launch of fs_importance_weights (its two launches, M = 1000),
              fs_weighted_reduce and fs_weighted_hist2d (M = 50,000, nb = 99, nr = 50) on the
              rows the reweighted batch stored, and of the per-batch energy and classify launches

Before timing, the keys the plain batch returns are compared bit for bit between the three
ways from one generator seed.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "flow-state_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from flowstate import _lib, analysis  # noqa: E402
from flowstate.MCMC import Physics  # noqa: E402
from flowstate.models import A2, build_flow, half_box  # noqa: E402


def window(fn, iters=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def summary(ts, **kw):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), windows=len(ts), **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    N = args.particles
    hb = half_box(N)
    phys = Physics(2 * hb)
    ways = {"plain": {}, "reweight": dict(reweight=phys), "reweight_density_pass": dict(reweight=phys,
                                                                                       density_pass=True)}
    with _lib.on_device(dev):
        torch.manual_seed(0)
        m = build_flow(N, bound=hb, device="cpu", **A2).to(dev).eval()
        m.q0.device = dev

        def batch(kw, seed=0):
            g = torch.Generator(device=dev).manual_seed(seed)
            return analysis.sample_analysis(m, args.samples, hb, generator=g, **kw)

        first = {k: batch(kw) for k, kw in ways.items()}  # also the warm-up
        for k in ("reweight", "reweight_density_pass"):
            for key in ("samples", "hist"):
                assert torch.equal(first[k][key], first["plain"][key]), (k, key)
            assert (first[k]["g_r"] == first["plain"]["g_r"]).all(), k
        times = {k: [] for k in ways}
        for _ in range(args.rounds):
            for k, kw in ways.items():
                times[k].append(window(lambda: batch(kw)))
        rw = first["reweight"]
        total = rw["samples"].shape[0]
        res = {"flow": f"A2, N={N}", "samples": total, "batch_rows": 1000,
               "batch": {k: summary(v) for k, v in times.items()},
               "weights": {k: rw[k] for k in ("ess", "ess_fraction", "log_z", "mean_log_w", "max_weight_fraction",
                                              "n_zero", "n_bad")}}

        # the launches one by one, on the rows the reweighted batch stored
        L, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
        samples, lw, E, lq = rw["samples"], rw["log_w"], rw["energy"], rw["log_q"]
        r_edges, denom, _ = analysis._rdf_bins(N, hb, hb / 50)
        nb, nr = 99, r_edges.shape[0] - 1
        e2 = torch.as_tensor(rw["x_edges"], device=dev)
        d = torch.as_tensor(denom, device=dev)
        counts = analysis.pair_histograms(samples - torch.tensor(hb, dtype=torch.float32), hb, r_edges)
        _, well, avg_x = analysis.classify_wells(samples, hb, 1.2)
        state = analysis.iw_state(dev)
        lw_b = torch.empty(1000, dtype=torch.float64, device=dev)
        E_b = torch.empty(1000, dtype=torch.float64, device=dev)
        g_w = torch.empty(nr, dtype=torch.float64, device=dev)
        sc = torch.empty(4, dtype=torch.float64, device=dev)
        hist_w = torch.zeros((nb, nb), dtype=torch.float64, device=dev)
        for i in range(0, total, 1000):  # a finished state over all rows for the two reductions
            _lib.check(L.fs_importance_weights(phys.beta, 1000, p(E[i:]), p(lq[i:]), p(lw_b), p(state), st))
        launches = {
            "fs_importance_weights (M=1000, 2 launches)":
                lambda: L.fs_importance_weights(phys.beta, 1000, p(E), p(lq), p(lw_b), p(state), st),
            f"fs_weighted_reduce (M={total})":
                lambda: L.fs_weighted_reduce(p(counts), total, nr, p(d), p(well), p(avg_x), p(lw), p(state), p(g_w),
                                             p(sc), st),
            f"fs_weighted_hist2d (M={total})":
                lambda: L.fs_weighted_hist2d(p(samples), total, N, hb, p(e2), nb, p(lw), p(state), p(hist_w), st),
            "fs_energy_lj_dw (M=1000)":
                lambda: L.fs_energy_lj_dw(phys.c, p(samples), 1, 1000, N, p(E_b), None, None, None, st),
            "fs_classify_wells (M=1000)":
                lambda: L.fs_classify_wells(p(samples), 1, 1000, N, hb, 1.2, None, p(well), p(avg_x), st),
        }
        # the same two reductions with equal weights: no row is skipped, every particle is binned
        # (an untrained flow's weights leave most rows at zero weight)
        state_eq, lw_eq = analysis.iw_state(dev), torch.empty(total, dtype=torch.float64, device=dev)
        zE, zq = torch.zeros(1000, dtype=torch.float64, device=dev), torch.zeros(1000, device=dev)
        for i in range(0, total, 1000):
            _lib.check(L.fs_importance_weights(phys.beta, 1000, p(zE), p(zq), p(lw_eq[i:]), p(state_eq), st))
        launches[f"fs_weighted_reduce (M={total}, equal weights)"] = \
            lambda: L.fs_weighted_reduce(p(counts), total, nr, p(d), p(well), p(avg_x), p(lw_eq), p(state_eq), p(g_w),
                                         p(sc), st)
        launches[f"fs_weighted_hist2d (M={total}, equal weights)"] = \
            lambda: L.fs_weighted_hist2d(p(samples), total, N, hb, p(e2), nb, p(lw_eq), p(state_eq), p(hist_w), st)
        res["launch"] = {}
        for name, fn in launches.items():
            assert fn() == 0, name
            window(fn, 10)
            res["launch"][name] = summary([window(fn, args.iters) for _ in range(args.rounds)], iters=args.iters)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
