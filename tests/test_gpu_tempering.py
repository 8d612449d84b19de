"""GPU tests of the temperature ladder (MCMC.TemperedMonteCarlo, fs_*_beta,
fs_replica_exchange).

1. Local moves: each rung's chains of a ladder launch are bit-identical to the same chains of
   a plain BatchedMonteCarlo at that rung's temperature, on the launcher's layouts and on a
   second FS_LOCAL_LAYOUT.
2. The same for fused NF-MH steps, with and without local moves before them (FS_MH_HYBRID).
3. fs_replica_exchange against the numpy statement (tempering_cases.exchange_round): the
   decisions, the exchanged arrays, what stays, the PCG64 streams, the counters, and the
   round-trip bookkeeping over 4 T rounds of always-accepted exchanges.
4. Exactness: the left-well population of one particle in the double well at four
   temperatures against quadrature, and the same engine without exchanges stuck in its well.
5. A sweeps() call captured into a graph equals the eager call.
"""
import numpy as np
import pytest
import torch

from flowstate import _lib
from flowstate.MCMC import BatchedMonteCarlo, Physics, TemperedMonteCarlo
from tempering_cases import (BOX, EXACT_MAX_DISP, EXACT_START, EXACT_TEMPERATURES, K, R0, V0, exchange_round,
                             initial_bookkeeping, p_left_exact, trip_bookkeeping)
from oracle import physics as OP
from test_gpu_local import G, _random_batch, _trace_model, _u64

pytestmark = pytest.mark.gpu

TEMPS = (0.7, 1.0, 1.5, 2.3)
T, R, C = 4, 8, 32
SEEDS = np.arange(1000, 1000 + C, dtype=np.uint64)


def _engines(N, model=None, seed=None):
    """The ladder engine and, per rung, the plain engine at that temperature, all over the
    same C chains (mixed float32 / float64 states)."""
    L, init, f32 = _random_batch(N, C, seed=N if seed is None else seed, spread=0.3)
    f32[:2] = [True, False]
    state = np.where(f32[:, None, None], init.astype(np.float32).astype(np.float64), init)

    def ready(b):
        b.state_is_f32.copy_(torch.from_numpy(f32.astype(np.uint8)))
        b.E_old, b.W_old = b._energy_of_state()
        return b

    lad = ready(TemperedMonteCarlo(model, state, Physics(L, L), SEEDS, TEMPS, initial_max_displacement=0.65))
    plain = [ready(BatchedMonteCarlo(model, state, Physics(L, L, temperature=t), SEEDS, initial_max_displacement=0.65))
             for t in TEMPS]
    return lad, plain


def _same_on_rung(lad, ref, t, names, extra=()):
    idx = torch.arange(t, C, T, device=lad.device)
    for name in names:
        a, b = getattr(lad, name)[idx], getattr(ref, name)[idx]
        assert torch.equal(a, b), f"rung {t}: {name} differs"
    for what, a, b in extra:
        assert torch.equal(a[idx], b[idx]), f"rung {t}: {what} differs"


LOCAL_NAMES = ("state", "E_old", "W_old", "pcg", "pcg_buf", "max_disp", "attempts", "accepted")


@pytest.mark.parametrize("N,layout", [(1, None), (3, None), (5, None), (16, None), (33, None), (64, None),
                                      (3, "8x1"), (64, "16x4")])
def test_ladder_local_moves_are_the_uniform_chains(N, layout, monkeypatch):
    if layout is None:
        monkeypatch.delenv("FS_LOCAL_LAYOUT", raising=False)
    else:
        monkeypatch.setenv("FS_LOCAL_LAYOUT", layout)
    lad, plain = _engines(N)
    assert (lad.R, lad.T) == (R, T) and lad.steps_per_launch() == 1
    assert torch.equal(lad.temperature_index.cpu(), torch.arange(C) % T)
    assert torch.equal(lad.beta_c.cpu(), torch.from_numpy(np.tile(1.0 / np.array(TEMPS), R)))
    assert lad.chains_at(2).tolist() == list(range(2, C, T))
    _, _, log = lad.local_moves(200, adjust_every=50, log_accepts=True)
    rates = []
    for t, ref in enumerate(plain):
        _, _, rlog = ref.local_moves(200, adjust_every=50, log_accepts=True)
        _same_on_rung(lad, ref, t, LOCAL_NAMES, extra=[("accept log", log, rlog)])
        rates.append(float(rlog.float().mean()))
    if N > 1:  # the temperatures matter: the plain engines do not all accept alike
        assert len(set(rates)) > 1, rates


STEP_NAMES = ("accept", "state", "state_is_f32", "E_old", "nll_old", "pcg", "attempts", "accepted")


@pytest.mark.parametrize("N", [3, 16])
def test_ladder_nf_steps_are_the_uniform_chains(N):
    f = np.load(G + "/local_trace.npz")
    model = _trace_model(N, f)
    lad, plain = _engines(N, model=model, seed=40 + N)
    program = [("step", 1), ("step", 1), ("step", 1), ("local", 20), ("step", 1)]  # the last one is hybrid
    got = []
    for what, n in program:
        if what == "local":
            lad.local_moves(n)
        else:
            lad.step(n)
            got.append({k: getattr(lad, k).clone() for k in STEP_NAMES})
    lad.check_errors()
    for t, ref in enumerate(plain):
        idx = torch.arange(t, C, T, device=lad.device)
        k = 0
        for what, n in program:
            if what == "local":
                ref.local_moves(n)
                continue
            ref.step(n)
            for name in STEP_NAMES:
                assert torch.equal(got[k][name][idx], getattr(ref, name)[idx]), f"rung {t}, step {k}: {name}"
            k += 1
    assert int(lad.attempts.min()) == 24  # 4 big moves + 20 local moves, shared counters


def exchange_states(N, Cx, seed):
    """Cx non-overlapping configurations spread widely enough (lattice + a jitter of 1.0) that
    their energies differ by several kT: the first Cx candidates the oracle finds finite."""
    L, init, f32 = _random_batch(N, 2 * Cx, seed=seed, spread=1.0)
    phys = OP.make_phys(N)  # finite as float32 and as float64 states
    E = OP.total_energy_batch(init.astype(np.float32), phys)[0] + OP.total_energy_batch(init, phys)[0]
    keep = np.flatnonzero(np.isfinite(E))[:Cx]
    assert len(keep) == Cx
    return L, init[keep], f32[keep]


def _exchange_case(N, seed):
    """R = 64 ladders of T = 5 rungs: non-overlapping random states with mixed dtype flags,
    their energies, one overlapping chain (E = +inf) and three equal energies in a row (a
    d = 0 pair at either parity)."""
    Tx, Rx = 5, 64
    Cx = Tx * Rx
    L, init, f32 = exchange_states(N, Cx, seed)
    state = np.where(f32[:, None, None], init.astype(np.float32).astype(np.float64), init)
    state[7, 1] = np.mod(state[7, 0] + 0.1, L)  # chain 7: a hard-core overlap
    b = BatchedMonteCarlo(None, state, Physics(L, L), np.arange(77, 77 + Cx, dtype=np.uint64))
    b.state_is_f32.copy_(torch.from_numpy(f32.astype(np.uint8)))
    E, W = b._energy_of_state()
    E[11] = E[10]
    E[12] = E[10]
    assert torch.isinf(E[7]) and int(torch.isfinite(E).sum()) == Cx - 1
    rng = np.random.default_rng(seed)
    nll = torch.from_numpy(rng.normal(0.0, 3.0, Cx)).to(b.device)
    return Tx, Rx, b, E, W, nll


def _call_exchange(Rx, Tx, N, parity, beta, dev):
    return _lib.load().fs_replica_exchange(Rx, Tx, N, parity, _lib.ptr(beta), _lib.ptr(dev["state"]),
                                           _lib.ptr(dev["state_is_f32"]), _lib.ptr(dev["E"]), _lib.ptr(dev["W"]),
                                           _lib.ptr(dev["nll"]), _lib.ptr(dev["pcg"]), _lib.ptr(dev["replica_id"]),
                                           _lib.ptr(dev["swap_attempts"]), _lib.ptr(dev["swap_accepts"]),
                                           _lib.ptr(dev["trip_dir"]), _lib.ptr(dev["round_trips"]),
                                           _lib.stream_ptr())


@pytest.mark.parametrize("N", [5, 64])
@pytest.mark.parametrize("parity", [0, 1])
def test_exchange_kernel_matches_the_numpy_statement(N, parity):
    Tx, Rx, b, E, W, nll = _exchange_case(N, seed=300 + N)
    Cx = Tx * Rx
    temps = np.array([0.7, 1.0, 1.5, 2.3, 3.5])
    beta_np = np.tile(1.0 / temps, Rx)
    beta = torch.from_numpy(beta_np).to(b.device)
    rid, trip, trips = initial_bookkeeping(Rx, Tx)
    dev = {"state": b.state.clone(), "state_is_f32": b.state_is_f32.clone(), "E": E.clone(), "W": W.clone(),
           "nll": nll.clone(), "pcg": b.pcg.clone(), "replica_id": torch.from_numpy(rid).to(b.device),
           "swap_attempts": torch.zeros(Cx, dtype=torch.int64, device=b.device),
           "swap_accepts": torch.zeros(Cx, dtype=torch.int64, device=b.device),
           "trip_dir": torch.from_numpy(trip).to(b.device), "round_trips": torch.from_numpy(trips).to(b.device)}
    # the draw each chain would take, from a copy of the streams
    pcg_next = b.pcg.clone()
    u = torch.empty(Cx, dtype=torch.float64, device=b.device)
    _lib.check(_lib.load().fs_pcg64_random(_lib.ptr(pcg_next), Cx, _lib.ptr(u), _lib.stream_ptr()), "fs_pcg64_random")
    want = {k: dev[k].cpu().numpy().copy() for k in ("state", "state_is_f32", "E", "W", "nll", "replica_id")}
    att, acc = np.zeros(Cx, np.int64), np.zeros(Cx, np.int64)
    i, accept, drew, d = exchange_round(Rx, Tx, parity, beta_np, want, u.cpu().numpy(), att, acc)
    trip_bookkeeping(Rx, Tx, parity, want["replica_id"], trip, trips)
    # no decision sits on the edge of the comparison
    un = u.cpu().numpy()[i][drew]
    ed = np.exp(d[drew])
    assert not np.any(np.abs(un - ed) < 1e-12 * ed)
    # the case exercises every branch: free accepts, drawn accepts, drawn rejects, the inf reject, d == 0
    assert (accept & ~drew).any() and (accept & drew).any() and (~accept & drew).any()
    assert (~accept & ~drew).sum() == 1 and np.isnan(d[~accept & ~drew]).all()  # the overlapping chain's pair
    forced = np.flatnonzero(i == 10 + parity)[0]  # chains 10, 11, 12 hold one energy
    assert d[forced] == 0.0 and accept[forced] and not drew[forced]

    _lib.check(_call_exchange(Rx, Tx, N, parity, beta, dev), "fs_replica_exchange")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev["swap_accepts"].cpu().numpy()[i].astype(bool), accept)  # the decisions
    for k, v in want.items():
        np.testing.assert_array_equal(dev[k].cpu().numpy(), v, err_msg=k)
    np.testing.assert_array_equal(dev["swap_attempts"].cpu().numpy(), att)
    np.testing.assert_array_equal(dev["swap_accepts"].cpu().numpy(), acc)
    np.testing.assert_array_equal(dev["trip_dir"].cpu().numpy(), trip)
    np.testing.assert_array_equal(dev["round_trips"].cpu().numpy(), trips)
    # the streams: one draw on the lower chain of each pair that drew, nothing elsewhere
    pcg_want = _u64(b.pcg).copy()
    pcg_want[i[drew]] = _u64(pcg_next)[i[drew]]
    np.testing.assert_array_equal(_u64(dev["pcg"]), pcg_want)
    assert torch.equal(beta.cpu(), torch.from_numpy(beta_np))


def test_exchange_round_trips_follow_the_labels():
    """All temperatures equal: d = 0, every exchange is accepted and the labels run the
    odd-even transposition; replica_id, trip_dir and round_trips after each of 4 T rounds."""
    N = 5
    Tx, Rx, b, E, W, nll = _exchange_case(N, seed=9)
    Cx = Tx * Rx
    E[7] = E[6]  # every energy finite
    beta = torch.ones(Cx, dtype=torch.float64, device=b.device)
    rid, trip, trips = initial_bookkeeping(Rx, Tx)
    dev = {"state": b.state.clone(), "state_is_f32": b.state_is_f32.clone(), "E": E.clone(), "W": W.clone(),
           "nll": nll.clone(), "pcg": b.pcg.clone(), "replica_id": torch.from_numpy(rid).to(b.device),
           "swap_attempts": torch.zeros(Cx, dtype=torch.int64, device=b.device),
           "swap_accepts": torch.zeros(Cx, dtype=torch.int64, device=b.device),
           "trip_dir": torch.from_numpy(trip).to(b.device), "round_trips": torch.from_numpy(trips).to(b.device)}
    want = {"E": E.cpu().numpy().copy(), "replica_id": rid, "state": b.state.cpu().numpy().copy()}
    for rnd in range(4 * Tx):
        _lib.check(_call_exchange(Rx, Tx, N, rnd % 2, beta, dev), "fs_replica_exchange")
        _, accept, drew, _ = exchange_round(Rx, Tx, rnd % 2, np.ones(Cx), want, np.ones(Cx))
        assert accept.all() and not drew.any()
        trip_bookkeeping(Rx, Tx, rnd % 2, rid, trip, trips)
        np.testing.assert_array_equal(dev["replica_id"].cpu().numpy(), rid, err_msg=f"round {rnd}")
        np.testing.assert_array_equal(dev["trip_dir"].cpu().numpy(), trip, err_msg=f"round {rnd}")
        np.testing.assert_array_equal(dev["round_trips"].cpu().numpy(), trips, err_msg=f"round {rnd}")
    np.testing.assert_array_equal(dev["state"].cpu().numpy(), want["state"])
    np.testing.assert_array_equal(_u64(dev["pcg"]), _u64(b.pcg))  # no draw was taken
    assert trips.sum() > 0 and (dev["swap_accepts"] == dev["swap_attempts"]).all()


def test_exchange_samples_the_right_distribution():
    """One particle in the double well, R = 4096 ladders over (0.5, 0.9, 1.6, 3.0), every
    chain started in the left well: after sweeps(400, 50) the fraction of ladders with
    x < L / 2 at each rung is within 5 binomial standard deviations of the exact value (the
    ladders are independent), while the same engine without exchanges is still in the left
    well at T = 0.5 (a 12 kT barrier; the numpy statement gives 0.999)."""
    Rx, Tx = 4096, len(EXACT_TEMPERATURES)
    Cx = Rx * Tx
    xy = np.tile(np.asarray(EXACT_START, dtype=np.float64), (Cx, 1, 1))
    seeds = np.arange(1000, 1000 + Cx, dtype=np.uint64)

    def engine():
        return TemperedMonteCarlo(None, xy, Physics(BOX, BOX, num_wells=2, V0_list=V0, r0=R0, k=K), seeds,
                                  EXACT_TEMPERATURES, initial_max_displacement=EXACT_MAX_DISP)

    lad = engine()
    lad.sweeps(400, 50)
    left = (lad.state[:, 0, 0].reshape(Rx, Tx) < BOX / 2).double().mean(0).cpu().numpy()
    still = engine()
    still.local_moves(400 * 50)
    left_still = (still.state[:, 0, 0].reshape(Rx, Tx) < BOX / 2).double().mean(0).cpu().numpy()
    exact = [p_left_exact(t) for t in EXACT_TEMPERATURES]
    bounds = [5.0 * np.sqrt(p * (1.0 - p) / Rx) for p in exact]
    print("P_left with exchange", left, "exact", exact, "bound", bounds, "without exchange", left_still)
    for t in range(Tx):
        assert abs(left[t] - exact[t]) <= bounds[t], (t, left[t], exact[t], bounds[t])
    assert left_still[0] > 0.9
    # the summary restates the raw counters
    s = lad.swap_summary()
    att = lad.swap_attempts.reshape(Rx, Tx).sum(0).cpu().numpy()
    acc = lad.swap_accepts.reshape(Rx, Tx).sum(0).cpu().numpy()
    assert s["R"] == Rx and s["T"] == Tx and s["exchange_rounds"] == 400 and len(s["pairs"]) == Tx - 1
    for t, pair in enumerate(s["pairs"]):
        assert pair["rungs"] == [t, t + 1] and pair["attempts"] == att[t] == 200 * Rx and pair["accepts"] == acc[t]
        assert pair["rate"] == acc[t] / att[t] and 0.0 < pair["rate"] < 1.0
    assert att[Tx - 1] == 0 and acc[Tx - 1] == 0
    trips = lad.round_trips.reshape(Rx, Tx).sum(1).cpu().numpy()
    assert s["round_trips"]["per_ladder"] == trips.tolist() and s["round_trips"]["total"] == trips.sum() > 0
    assert int(lad.round_trips.sum()) > 0
    for t, rung in enumerate(s["temperatures"]):
        assert rung["temperature"] == EXACT_TEMPERATURES[t] and rung["well_samples"] == Rx
        assert rung["mean_E"] == pytest.approx(float(lad.E_old.reshape(Rx, Tx)[:, t].mean()), rel=1e-12)
        assert rung["acceptance"] == float(lad.accepted.reshape(Rx, Tx)[:, t].sum()) / (Rx * 400 * 50)
    assert torch.equal(lad.replica_id.reshape(Rx, Tx).sort(1).values.cpu(),
                       torch.arange(Tx, dtype=torch.int32).expand(Rx, Tx))
    # one-beta calls are refused
    with pytest.raises(NotImplementedError):
        lad.metropolis_judge(lad.E_old, lad.E_old[:, None])
    with pytest.raises(NotImplementedError):
        lad.judge_normalizing_flow(lad.state)
    with pytest.raises(NotImplementedError):
        lad.bulk_judge_normalizing_flow(lad.state[:, None], 0.0)


def test_ladder_sweeps_in_a_captured_graph():
    N = 16
    L, init, _ = _random_batch(N, C, seed=5, spread=0.3)
    names = LOCAL_NAMES + ("state_is_f32", "replica_id", "swap_attempts", "swap_accepts", "trip_dir", "round_trips")

    def engine():
        return TemperedMonteCarlo(None, init, Physics(L, L), SEEDS, TEMPS, initial_max_displacement=0.65)

    eager = engine()
    eager.sweeps(3, 40, adjust_every=20)
    graphed = engine()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.sweeps(3, 40, adjust_every=20)
    before = graphed.attempts.clone()
    assert int(before.sum()) == 0  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    for name in names:
        assert torch.equal(getattr(graphed, name), getattr(eager, name)), name
    assert int(eager.swap_attempts.sum()) == R * (2 + 1 + 2)
    # a graph of an even number of rounds whose moves end on the adjust schedule continues the
    # alternation on every replay: two replays of two rounds are four eager rounds
    eager4, twice = engine(), engine()
    eager4.sweeps(4, 40, adjust_every=20)
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        twice.sweeps(2, 40, adjust_every=20)
    g2.replay()
    g2.replay()
    torch.cuda.synchronize()
    for name in names:
        assert torch.equal(getattr(twice, name), getattr(eager4, name)), name


def test_gated_ladder_local_moves():
    """fs_local_moves_beta with a gate (the _if form): gate 0 changes nothing, gate 1 is the
    ungated ladder launch."""
    N = 16
    lad, _ = _engines(N, seed=61)
    ref, _ = _engines(N, seed=61)
    names = LOCAL_NAMES + ("prev_counts",)
    before = {k: getattr(lad, k).clone() for k in names}
    gate = torch.zeros(1, dtype=torch.uint8, device=lad.device)

    def gated(b):
        _lib.check(_lib.load().fs_local_moves_beta(
            _lib.ptr(b.beta_c), b.phys.c, b.C, b.N, _lib.ptr(b.state), _lib.ptr(b.state_is_f32), _lib.ptr(b.E_old),
            _lib.ptr(b.W_old), _lib.ptr(b.pcg), _lib.ptr(b.pcg_buf), _lib.ptr(b.max_disp), _lib.ptr(b.attempts),
            _lib.ptr(b.accepted), _lib.ptr(b.prev_counts), 100, 0, 50, b.target_acceptance, 0, None, None, None, None,
            _lib.ptr(gate), _lib.stream_ptr()), "fs_local_moves_beta")

    gated(lad)
    for k in names:
        assert torch.equal(getattr(lad, k), before[k]), f"gate 0 changed {k}"
    gate.fill_(1)
    gated(lad)
    ref.local_moves(100, adjust_every=50)
    for k in names:
        assert torch.equal(getattr(lad, k), getattr(ref, k)), f"gate 1: {k}"
    assert int(lad.attempts.min()) == 100
