"""Density and sampling pass times of the general-shape mode ("f32-general") beside the
default mode's instantiated kernels, in one process on the MI355X (DESIGN.md
'General-shape mode').  Event-timed: every (shape, rows, mode, pass) is warmed up, then
timed over at least 20 passes in 3 rounds that alternate the modes; the median round is
reported with the spread.  Rates are the algorithmic conditioner FLOP (oracle.flow /
bench.flops_per_pass) over the pass time, as a fraction of the dense f32 MFMA peak.

    python tools/general_ab.py [--out results.json]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "flow-state_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from flowstate.models import A1, A2, build_flow, half_box  # noqa: E402

PEAK_F32_TFLOPS = 157.3  # MI355X dense FP32 MFMA (bench.py)


def flops_per_pass(N, L, H, nb, K):
    return 2 * L * (2 * N * H + 2 * nb * H * H + H * N * (3 * K + 1))


def model(N, kw):
    """Random-init flow with non-trivial final layers and unconditional logits (bench.synthetic_model's recipe)."""
    torch.manual_seed(0)
    m = build_flow(N, **kw)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for f in m.flows:
            w = f.prqct.transform_net.final_layer.weight
            w.copy_(torch.randn(w.shape, generator=g) * 0.01)
            u = f.prqct.unconditional_transform
            u.unnormalized_widths.copy_(torch.randn(u.unnormalized_widths.shape, generator=g) * 0.3)
            u.unnormalized_heights.copy_(torch.randn(u.unnormalized_heights.shape, generator=g) * 0.3)
    return m.cuda().eval()


def time_pass(fn, min_passes=20, window_s=0.25):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        fn()
    b.record()
    torch.cuda.synchronize()
    per = a.elapsed_time(b) / 5 / 1e3
    n = int(min(5000, max(min_passes, window_s / max(per, 1e-7))))
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n / 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    cases = [("A2", 64, dict(A2), ("f32", "f32-general")), ("A1", 64, dict(A1), ("f32", "f32-general")),
             ("H96_K10", 64, dict(L=23, H=96, nb=2, K=10), ("f32-general",)),
             ("H512_K32", 64, dict(L=15, H=512, nb=4, K=32), ("f32-general",))]
    results = []
    for name, N, kw, modes in cases:
        m = model(N, kw)
        B = half_box(N)
        for rows in (4096, 65536):
            x = ((torch.rand((rows, 2 * N), device="cuda") * 2 - 1) * B).contiguous()
            fl = flops_per_pass(N, **kw) * rows
            rec = {"case": name, "N": N, **kw, "rows": rows}
            outs = {}
            times = {(md, ps): [] for md in modes for ps in ("density", "sample")}
            for rnd in range(3):
                for md in modes:  # alternate the modes inside every round
                    m.set_precision(md)
                    outs[md] = (m.log_prob(x), m.forward(x))
                    times[(md, "density")].append(time_pass(lambda: m.log_prob(x))[0])
                    times[(md, "sample")].append(time_pass(lambda: m.forward(x))[0])
            for (md, ps), ts in times.items():
                ts = sorted(ts)
                rec[f"{md}/{ps}"] = {"s": ts[1], "min_s": ts[0], "max_s": ts[2], "tflops": fl / ts[1] / 1e12,
                                     "mfma_frac": fl / ts[1] / 1e12 / PEAK_F32_TFLOPS}
            if len(modes) == 2:
                for ps in ("density", "sample"):
                    rec[f"slowdown/{ps}"] = rec[f"f32-general/{ps}"]["s"] / rec[f"f32/{ps}"]["s"]
                lq0, lq1 = outs["f32"][0].double(), outs["f32-general"][0].double()
                fin = torch.isfinite(lq0)
                rec["max_rel_dlogq"] = float(((lq0 - lq1).abs()[fin] / lq0.abs()[fin]).max())
                rec["max_dx_over_B"] = float((outs["f32"][1] - outs["f32-general"][1]).abs().max() / B)
            print(json.dumps(rec), flush=True)
            results.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
