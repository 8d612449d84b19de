"""TemperedMonteCarlo — a temperature ladder over the chains of a BatchedMonteCarlo, with
replica exchange (parallel tempering).  Not in the reference, which runs one process per
temperature and has local moves and flow proposals only.

Layout: C = R T chains, chain c = r T + t is rung t of ladder r and runs at
beta_c[c] = 1 / temperatures[t] (temperatures strictly increasing).  A chain index is a
temperature: everything that is per chain on a BatchedMonteCarlo (the tuned max_disp, the
attempt / accept counters, a ChainRecorder's series, well_counts, histogram2d) is per
temperature here, and an accepted exchange moves the configurations (state, its dtype flag,
E_old, W_old, nll_old and the label replica_id), never the temperatures.

The local moves and the big moves read the chain's own beta in their accept and are
otherwise the plain engine's kernels: a chain of a ladder runs bit for bit as the same chain
of a BatchedMonteCarlo at that temperature (fs_local_moves_beta, fs_nf_mh_step_beta,
fs_mh_accept_beta).  A flow proposal's log q does not depend on beta, so a big move judged
with the chain's beta is a valid Metropolis-Hastings move on every rung.
fs_replica_exchange is one exchange round (include/flowstate.h states the rule).

Not on a ladder engine (each raises NotImplementedError): metropolis_judge,
judge_normalizing_flow and bulk_judge_normalizing_flow (they take one scalar beta), and the
drivers built on one beta: algorithm1.testing_phase and Algorithm2.

Still one scalar beta, and therefore wrong on a ladder unless taken rung by rung with the
rung's own temperature: everything that reads `physics.beta` (the Physics object's
temperature, 1.0 by default, which no accept of this engine uses).  That is the `beta` a
diagnostics.ChainRecorder hands to diagnose() (its pressure_mean, and its statistics pooled
over all chains, which here mix the temperatures: select a rung's columns with chains_at(t)),
the beta column of io.sample_tuples / algorithm1.Snapshots, and
analysis.sample_analysis(reweight=physics).
"""
import numpy as np
import torch

from .. import _lib
from .batched import BatchedMonteCarlo, _on_own_device


def ladder_layout(C, temperatures):
    """(R, T, temperatures (T,) f64, beta_c (C,) f64, temperature_index (C,) int64) of C chains
    over a ladder: T >= 2 finite, positive, strictly increasing temperatures and C a multiple
    of T; chain r T + t is rung t of ladder r.  ValueError otherwise."""
    temps = np.asarray(temperatures, dtype=np.float64).reshape(-1)
    T = int(temps.size)
    if T < 2:
        raise ValueError(f"a temperature ladder needs at least 2 temperatures, got {T}")
    if not np.all(np.isfinite(temps)) or temps[0] <= 0.0:
        raise ValueError("temperatures must be positive and finite")
    if not np.all(np.diff(temps) > 0.0):
        raise ValueError("temperatures must be strictly increasing")
    C = int(C)
    if C <= 0 or C % T != 0:
        raise ValueError(f"{C} chains are not whole ladders of {T} temperatures (C % T != 0)")
    index = np.arange(C, dtype=np.int64) % T
    return C // T, T, temps, 1.0 / temps[index], index


def _no_ladder(what):
    raise NotImplementedError(f"{what} takes one scalar beta and is not available on a temperature ladder "
                              "(TemperedMonteCarlo); use one BatchedMonteCarlo per temperature for it")


class TemperedMonteCarlo(BatchedMonteCarlo):
    is_ladder = True  # algorithm1.testing_phase and Algorithm2 refuse such an engine

    def __init__(self, model, particles, physics, seeds, temperatures, **kwargs):
        """particles (C, N, 2) with C = R len(temperatures), chain r T + t on rung t; physics:
        the box and wells (its own temperature is not used by the accepts); the other
        arguments are BatchedMonteCarlo's."""
        shape = tuple(particles.shape) if hasattr(particles, "shape") else np.asarray(particles).shape
        C = 1 if len(shape) == 2 else int(shape[0])
        self.R, self.T, temps, beta, index = ladder_layout(C, temperatures)
        self.temperatures = temps
        super().__init__(model, particles, physics, seeds, **kwargs)
        dev = self.device
        self.beta_c = torch.as_tensor(beta, device=dev)
        self.temperature_index = torch.as_tensor(index, device=dev)
        self.replica_id = self.temperature_index.to(torch.int32)
        self.swap_attempts = torch.zeros(self.C, dtype=torch.int64, device=dev)
        self.swap_accepts = torch.zeros(self.C, dtype=torch.int64, device=dev)
        self.trip_dir = (self.temperature_index == 0).to(torch.int8)  # label 0 has been at rung 0
        self.round_trips = torch.zeros(self.C, dtype=torch.int64, device=dev)
        self.exchange_rounds = 0
        self._sweep_moves = 0  # local moves run by sweeps(): the adjust_every schedule's counter

    def chains_at(self, t):
        """The chain indices (R,) of rung t, one per ladder."""
        if not 0 <= int(t) < self.T:
            raise IndexError(f"rung {t} outside 0..{self.T - 1}")
        return torch.arange(int(t), self.C, self.T, device=self.device)

    # ------------------------------------------------------------------ moves at the chain's own beta
    def _launch_local_moves(self, L, n, step0, adjust_every, sample_every, sxy, sew, log):
        _lib.check(L.fs_local_moves_beta(_lib.ptr(self.beta_c), self.phys.c, self.C, self.N, _lib.ptr(self.state),
                                         _lib.ptr(self.state_is_f32), _lib.ptr(self.E_old), _lib.ptr(self.W_old),
                                         _lib.ptr(self.pcg), _lib.ptr(self.pcg_buf), _lib.ptr(self.max_disp),
                                         _lib.ptr(self.attempts), _lib.ptr(self.accepted),
                                         _lib.ptr(self.prev_counts), n, step0, adjust_every, self.target_acceptance,
                                         sample_every, _lib.ptr(sxy), _lib.ptr(sew), _lib.ptr(log), None, None,
                                         _lib.stream_ptr()), "fs_local_moves_beta")

    def _launch_mh_accept(self, L, E_new, W_new, lq, cfg):
        _lib.check(L.fs_mh_accept_beta(_lib.ptr(self.beta_c), self.phys.c, self.C, self.N, _lib.ptr(self.E_old),
                                       _lib.ptr(self.W_old), _lib.ptr(self.nll_old), _lib.ptr(E_new),
                                       _lib.ptr(W_new), _lib.ptr(lq), _lib.ptr(self.pcg), _lib.ptr(self.state),
                                       _lib.ptr(self.state_is_f32), _lib.ptr(cfg), _lib.ptr(self.accept),
                                       _lib.ptr(self.attempts), _lib.ptr(self.accepted), _lib.ptr(self.n_accept),
                                       self.flags, _lib.stream_ptr()), "fs_mh_accept_beta")

    def steps_per_launch(self):
        """A ladder engine runs one fused step per launch (no multi-step launch, no bank)."""
        return 1

    def _launch_fused_step(self, L, dims, packed, flags, st):
        """step()'s fused launch with each chain judged at its own beta (fs_nf_mh_step_beta);
        with steps_per_launch() == 1 the base step() takes no other path."""
        _lib.check(L.fs_nf_mh_step_beta(_lib.ptr(self.beta_c), dims, _lib.ptr(packed), self.phys.c, self.C,
                                        self.proposal_seed, self.step_count, self.chain_offset,
                                        _lib.ptr(self.E_old), _lib.ptr(self.W_old), _lib.ptr(self.nll_old),
                                        _lib.ptr(self.pcg), _lib.ptr(self.state), _lib.ptr(self.state_is_f32),
                                        _lib.ptr(self.accept), _lib.ptr(self.attempts), _lib.ptr(self.accepted),
                                        _lib.ptr(self.n_accept), _lib.ptr(self.err), flags,
                                        _lib.ptr(self._workspace()), st), "fs_nf_mh_step_beta")

    # ------------------------------------------------------------------ exchange
    @_on_own_device
    def replica_exchange(self, parity=None):
        """One exchange round (fs_replica_exchange): rungs (t, t + 1) for t = parity,
        parity + 2, ... of every ladder.  parity None alternates 0, 1, 0, ... from the
        engine's round counter.  The cached E_old / W_old / nll_old travel with the
        configurations, so they stay as exact as they were.  Stream-ordered, no host sync."""
        if parity is None:
            parity = self.exchange_rounds % 2
        _lib.check(_lib.load().fs_replica_exchange(self.R, self.T, self.N, int(parity), _lib.ptr(self.beta_c),
                                                   _lib.ptr(self.state), _lib.ptr(self.state_is_f32),
                                                   _lib.ptr(self.E_old), _lib.ptr(self.W_old),
                                                   _lib.ptr(self.nll_old), _lib.ptr(self.pcg),
                                                   _lib.ptr(self.replica_id), _lib.ptr(self.swap_attempts),
                                                   _lib.ptr(self.swap_accepts), _lib.ptr(self.trip_dir),
                                                   _lib.ptr(self.round_trips), _lib.stream_ptr()),
                   "fs_replica_exchange")
        self.exchange_rounds += 1

    @_on_own_device
    def sweeps(self, rounds, moves_per_round, big_moves_per_round=0, adjust_every=0):
        """rounds x (moves_per_round local moves, big_moves_per_round fused NF-MH steps, one
        exchange round), all on the current stream with no host synchronisation (so a call
        can be captured into a graph once the flow's workspace exists).  adjust_every:
        adjust_displacement on the schedule of the local moves run by sweeps() so far.
        The parities, the adjust schedule's step numbers and the proposal steps are host
        values fixed when the launches are issued: a captured graph repeats exactly the
        captured ones on every replay, and the host counters (exchange_rounds, step_count)
        count the capture only.  For replays that continue the alternation, capture an even
        number of rounds with moves_per_round a multiple of adjust_every; big moves in a
        replayed graph would repeat their proposals, so capture none."""
        for _ in range(int(rounds)):
            self.local_moves(int(moves_per_round), adjust_every=int(adjust_every), step0=self._sweep_moves)
            self._sweep_moves += int(moves_per_round)
            if big_moves_per_round:
                self.step(int(big_moves_per_round))
            self.replica_exchange()

    @_on_own_device
    def swap_summary(self, counts=None):
        """Host summary (plain floats, ints and lists; synchronises).  pairs: per rung pair
        (t, t + 1) the exchange attempts, accepts and rate summed over ladders; round_trips:
        per ladder and in total; temperatures: per rung the mean running energy over its
        finite chains, the acceptance of the moves counted in attempts / accepted (the local
        moves, and the big moves when some ran: the reference's shared counters) and the well
        populations from well_counts (counts: accumulated (C, 3) well_counts, default those
        of the current states)."""
        R, T = self.R, self.T
        att = self.swap_attempts.reshape(R, T).sum(0).cpu().numpy()
        acc = self.swap_accepts.reshape(R, T).sum(0).cpu().numpy()
        trips = self.round_trips.reshape(R, T).sum(1).cpu().numpy()
        E = self.E_old.reshape(R, T).cpu().numpy()
        a = self.attempts.reshape(R, T).sum(0).cpu().numpy()
        ok = self.accepted.reshape(R, T).sum(0).cpu().numpy()
        wc = (self.well_counts() if counts is None else counts).reshape(R, T, 3).sum(0).cpu().numpy()
        pairs = [{"rungs": [t, t + 1], "temperatures": [float(self.temperatures[t]), float(self.temperatures[t + 1])],
                  "attempts": int(att[t]), "accepts": int(acc[t]),
                  "rate": float(acc[t]) / float(att[t]) if att[t] else 0.0} for t in range(T - 1)]
        rungs = []
        for t in range(T):
            fin = np.isfinite(E[:, t])
            n = int(wc[t, 2])
            rungs.append({"temperature": float(self.temperatures[t]),
                          "mean_E": float(E[fin, t].mean()) if fin.any() else None,
                          "acceptance": float(ok[t]) / float(a[t]) if a[t] else 0.0,
                          "p_a": float(wc[t, 0]) / n if n else 0.0, "p_b": float(wc[t, 1]) / n if n else 0.0,
                          "well_samples": n})
        return {"R": R, "T": T, "exchange_rounds": int(self.exchange_rounds), "pairs": pairs,
                "round_trips": {"per_ladder": [int(v) for v in trips], "total": int(trips.sum())},
                "temperatures": rungs}

    # ------------------------------------------------------------------ one-beta calls
    def metropolis_judge(self, E_ref, E_new):
        _no_ladder("metropolis_judge")

    def judge_normalizing_flow(self, configs):
        _no_ladder("judge_normalizing_flow")

    def bulk_judge_normalizing_flow(self, configs, ref_energy):
        _no_ladder("bulk_judge_normalizing_flow")
