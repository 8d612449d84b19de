"""Cost of a temperature ladder (MCMC.TemperedMonteCarlo) beside the plain engine.

For `--chains` chains of N particles over `--rungs` temperatures, one JSON line with
  * the kernel time of `--moves` local moves per chain on a plain BatchedMonteCarlo (one
    beta) and on the ladder engine (fs_local_moves_beta), HIP events, mean of `--steps`;
  * the time of one exchange round (fs_replica_exchange, mean over `--rounds` rounds of
    alternating parity after the moves above), its accept rate, and the HBM traffic of the
    accepted rows (two rows of 2 N doubles read and written per accepted pair) as a fraction
    of `--peak-gbs`.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "flow-state_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from flowstate.MCMC import BatchedMonteCarlo, Physics, TemperedMonteCarlo, initialise_fcc  # noqa: E402


def timed(fn, steps):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in evs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in evs]
    return float(np.mean(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--rungs", type=int, default=8)
    ap.add_argument("--moves", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--t-min", type=float, default=0.7)
    ap.add_argument("--t-max", type=float, default=2.0)
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="HBM peak the traffic is reported against")
    args = ap.parse_args()
    N, C, T = args.particles, args.chains, args.rungs
    base, box = initialise_fcc(num_particles=N, rho=0.03, aspect_ratio=1.0)
    L = float(box.box_size_x)
    init = np.mod(base[None] + np.random.default_rng(7).normal(0, 0.05, (C, N, 2)), L)
    seeds = np.arange(42, 42 + C, dtype=np.uint64)
    temps = np.geomspace(args.t_min, args.t_max, T)
    plain = BatchedMonteCarlo(None, init, Physics(L, L), seeds, initial_max_displacement=0.65)
    lad = TemperedMonteCarlo(None, init, Physics(L, L), seeds, temps, initial_max_displacement=0.65)
    for b in (plain, lad):
        b.local_moves(args.moves)
    torch.cuda.synchronize()
    uni = timed(lambda: plain.local_moves(args.moves), args.steps)
    ldr = timed(lambda: lad.local_moves(args.moves), args.steps)
    lad.replica_exchange()
    lad.replica_exchange()
    a0, c0 = int(lad.swap_attempts.sum()), int(lad.swap_accepts.sum())
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(args.rounds):
        lad.replica_exchange()
    ev1.record()
    torch.cuda.synchronize()
    us = ev0.elapsed_time(ev1) * 1e3 / args.rounds
    att, acc = int(lad.swap_attempts.sum()) - a0, int(lad.swap_accepts.sum()) - c0
    moved = acc / args.rounds * 64.0 * N  # bytes per round: 2 rows x 2N doubles, read and written
    print(json.dumps({
        "metric": "temperature ladder: local moves and one exchange round", "particles": N, "chains": C, "rungs": T,
        "temperatures": [float(t) for t in temps], "moves_per_launch": args.moves,
        "uniform_local_ms": {"mean": uni[0], "min": uni[1], "max": uni[2]},
        "ladder_local_ms": {"mean": ldr[0], "min": ldr[1], "max": ldr[2]},
        "ladder_over_uniform": ldr[0] / uni[0],
        "one_local_move_of_the_batch_us": ldr[0] * 1e3 / args.moves,
        "exchange_round_us": us, "exchange_rounds_timed": args.rounds, "exchange_accept_rate": acc / max(att, 1),
        "exchange_bytes_per_round": moved, "exchange_gbs": moved / (us * 1e-6) / 1e9,
        "exchange_fraction_of_peak": moved / (us * 1e-6) / 1e9 / args.peak_gbs, "peak_gbs": args.peak_gbs,
    }), flush=True)


if __name__ == "__main__":
    main()
