"""Timings of the Algorithm-2 checkpoint cycle's analysis batch (main_algorithm_2.py:
485-525) on the device, by device events:

  fused      one fs_sample_analysis launch at M = 1000, N = 64, nb = 99, nr = 50
  composed   the same results from torch ops and the older kernels: float32 add,
             float32 subtract, a float64 copy, fs_hist2d, fs_pair_hist (5 launches)
  batch      analysis.sample_analysis on the A2 flow (L=23, H=128, 2 blocks, K=15),
             N = 64: 50 x (base draws + sampling pass + fs_sample_analysis) + fs_rdf_mean,
             results copied to the host at the end

The fused and composed results are compared (they must be identical) before timing.
Prints one JSON line."""
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

from flowstate import _lib, analysis  # noqa: E402
from flowstate.models import A2, build_flow, half_box  # noqa: E402


def timed(fn, iters, repeats):
    """ms per call: `repeats` windows of `iters` back-to-back calls between two events."""
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "iters": iters,
            "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-batch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    L = _lib.load()
    M, N = args.rows, args.particles
    hb = half_box(N)
    r_edges, _, _ = analysis._rdf_bins(N, hb, hb / 50)
    e2 = torch.from_numpy(np.linspace(-hb, hb, 100)).to(dev)
    er = torch.from_numpy(r_edges).to(dev)
    nb, nr = 99, r_edges.shape[0] - 1
    # samples crowded into the two wells, as a trained flow's are
    g = torch.Generator(device=dev).manual_seed(0)
    centre = torch.tensor([[-hb / 2, 0.0], [hb / 2, 0.0]], device=dev)[torch.randint(0, 2, (M, 1), device=dev,
                                                                                    generator=g)]
    z = (centre + 1.5 * torch.randn((M, N, 2), device=dev, generator=g)).clamp(-hb, hb).float().contiguous()
    out = torch.empty_like(z)
    hist = torch.zeros((nb, nb), dtype=torch.int64, device=dev)
    counts = torch.empty((M, nr), dtype=torch.int32, device=dev)
    hist_c = torch.zeros_like(hist)
    counts_c = torch.empty_like(counts)

    def fused():
        analysis.sample_analysis_batch(z, hb, e2, er, out, hist, counts)

    def composed():
        s = z + hb
        c = s - hb
        c64 = c.double()
        _lib.check(L.fs_hist2d(_lib.ptr(c64), M, N, 0.0, _lib.ptr(e2), nb, _lib.ptr(hist_c), _lib.stream_ptr()),
                   "fs_hist2d")
        _lib.check(L.fs_pair_hist(_lib.ptr(c), 1, M, N, float(hb), _lib.ptr(er), nr, _lib.ptr(counts_c),
                                  _lib.stream_ptr()), "fs_pair_hist")
        return s

    with _lib.on_device(dev):
        fused()
        s = composed()
        torch.cuda.synchronize()
        assert torch.equal(out, s) and torch.equal(hist, hist_c) and torch.equal(counts, counts_c)
        for _ in range(20):
            fused()
            composed()
        res = {"shape": {"M": M, "N": N, "nb": nb, "nr": nr},
               "fused": dict(timed(fused, args.iters, args.repeats), launches=1),
               "composed": dict(timed(composed, args.iters, args.repeats), launches=5)}
        if not args.skip_batch:
            torch.manual_seed(0)
            m = build_flow(N, bound=hb, device="cpu", **A2).to(dev).eval()
            m.q0.device = dev
            n_iter = -(-args.samples // 1000)

            def batch():
                analysis.sample_analysis(m, args.samples, hb, generator=g)

            batch()
            res["batch"] = dict(timed(batch, 1, args.repeats), samples=n_iter * 1000,
                                launches_analysis=n_iter + 1, flow=f"A2, N={N}")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
