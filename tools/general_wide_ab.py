"""Density and sampling pass times of the general-shape mode ("f32-general") on its wide
path (csrc/flow_general_kernels.hip "Wide path") beside flow_general_kernel, in one process
on the MI355X (DESIGN.md 'General-shape mode').  Event-timed: every (shape, rows, pass) is
warmed up, then timed over at least 20 passes in 3 rounds that alternate
fs_set_general_wide_rows(0) and (65536); the median round is reported with the spread.
fs_general_wide_passes must advance in the wide rounds only (where the wide path can run:
the fused grid below twice the compute units).  The last line names the largest row count
at which the wide path wins every shape and direction by more than the round-to-round
spread: the library's default limit.

    python tools/general_wide_ab.py [--out results.json]
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

from flowstate import _lib  # noqa: E402
from flowstate.models import A1, A2, half_box  # noqa: E402
from general_ab import model, time_pass  # noqa: E402

ROWS = (16, 256, 1024, 4096, 8192, 16384)
CASES = [("A2", 64, dict(A2)), ("A1", 64, dict(A1)), ("H96_K10", 64, dict(L=23, H=96, nb=2, K=10)),
         ("H512_K32", 64, dict(L=15, H=512, nb=4, K=32)), ("N3_H96_K10", 3, dict(L=15, H=96, nb=2, K=10))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    L = _lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    start = L.fs_set_general_wide_rows(-1)
    results = []
    wins = {rows: True for rows in ROWS}
    try:
        for name, N, kw in CASES:
            m = model(N, kw).set_precision("f32-general")
            B = half_box(N)
            fused_rows = 64 if kw["H"] <= 256 else 32
            for rows in ROWS:
                x = ((torch.rand((rows, 2 * N), device="cuda") * 2 - 1) * B).contiguous()
                can_wide = -(-rows // fused_rows) < 2 * cus
                rec = {"case": name, "N": N, **kw, "rows": rows, "wide_runs": can_wide}
                times = {(path, ps): [] for path in ("fused", "wide") for ps in ("density", "sample")}
                outs = {}
                # the passes through the C ABI on preallocated outputs: no host
                # synchronisation or allocation inside the timed loop
                dims, packed, st = m.dims(), m.packed(), _lib.stream_ptr()
                out, ld = torch.empty_like(x), torch.empty(rows, device="cuda")
                err = torch.zeros(1, dtype=torch.int32, device="cuda")
                p = _lib.ptr

                def density():
                    _lib.check(L.fs_flow_log_prob(dims, p(packed), p(x), rows, p(ld), p(out), p(err), st))

                def sample():
                    _lib.check(L.fs_flow_forward(dims, p(packed), p(x), rows, p(out), p(ld), p(err), st))

                for rnd in range(3):
                    for path, limit in (("fused", 0), ("wide", 65536)):  # alternate inside every round
                        L.fs_set_general_wide_rows(limit)
                        n0 = L.fs_general_wide_passes()
                        density()
                        lq = ld.clone()
                        sample()
                        outs[path] = (lq, out.clone())
                        times[(path, "density")].append(time_pass(density)[0])
                        times[(path, "sample")].append(time_pass(sample)[0])
                        advanced = L.fs_general_wide_passes() > n0
                        assert advanced == (path == "wide" and can_wide), (name, rows, path, advanced)
                assert torch.equal(outs["fused"][0], outs["wide"][0]) and torch.equal(outs["fused"][1], outs["wide"][1])
                assert int(err.item()) == 0
                for (path, ps), ts in times.items():
                    ts = sorted(ts)
                    rec[f"{path}/{ps}"] = {"s": ts[1], "min_s": ts[0], "max_s": ts[2]}
                for ps in ("density", "sample"):
                    f, w = rec[f"fused/{ps}"], rec[f"wide/{ps}"]
                    rec[f"speedup/{ps}"] = f["s"] / w["s"]
                    # a win: the wide path's slowest round beats the fused kernel's fastest
                    rec[f"wins/{ps}"] = bool(can_wide and w["max_s"] < f["min_s"])
                    wins[rows] = wins[rows] and rec[f"wins/{ps}"]
                print(json.dumps(rec), flush=True)
                results.append(rec)
    finally:
        L.fs_set_general_wide_rows(start)
    limit = max([rows for rows in ROWS if wins[rows]], default=0)
    print(json.dumps({"wins_by_rows": wins, "default_limit": limit}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"results": results, "wins_by_rows": wins, "default_limit": limit}, f, indent=1)


if __name__ == "__main__":
    main()
