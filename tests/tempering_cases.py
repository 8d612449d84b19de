"""Shared statements of the replica-exchange tests (test_tempering_cpu.py,
test_gpu_tempering.py), in numpy:

  exchange_round    one round of fs_replica_exchange on arrays, the uniform draws supplied;
  trip_bookkeeping  the round-trip bookkeeping that follows a round;
  well_energy / sample_ladders   the N = 1 double-well system of the exactness test and a
                    vectorised sampler of it with the engine's local-move rule;
  p_left_exact      the exact left-half probability by midpoint quadrature.
"""
import numpy as np

# the exactness system: one particle in the double well (Physics(8, 8, num_wells=2, ...))
BOX = 8.0
V0 = (-6.0, -7.0)
R0, K = 1.0, 10.0
EXACT_TEMPERATURES = (0.5, 0.9, 1.6, 3.0)
EXACT_START = (2.0, 4.0)
EXACT_MAX_DISP = 2.0
SWAPPED = ("state", "state_is_f32", "E", "W", "nll", "replica_id")  # what an accepted pair exchanges


def pair_lower_chains(R, T, parity):
    """The lower chain i = r T + t of every pair of a round: t = parity, parity + 2, ... < T - 1."""
    t = np.arange(parity, T - 1, 2)
    return (np.arange(R)[:, None] * T + t[None, :]).reshape(-1)


def exchange_round(R, T, parity, beta_c, arrays, u, swap_attempts=None, swap_accepts=None):
    """One exchange round, in place on `arrays` (a dict with "E" and any of SWAPPED, each
    indexed by chain on axis 0).  u [C]: the Generator.random() draw chain i would take.
    In double, in this order: E_i or E_j not finite rejects with no draw; d = (beta_i -
    beta_j)(E_i - E_j) >= 0 accepts with no draw; else accept iff u_i < exp(d).
    Returns (i, accept, drew, d): the lower chains, and per pair the decision, whether it
    drew, and d (NaN where an energy is not finite)."""
    i = pair_lower_chains(R, T, parity)
    j = i + 1
    E = arrays["E"]
    finite = np.isfinite(E[i]) & np.isfinite(E[j])
    with np.errstate(invalid="ignore"):
        d = np.where(finite, (beta_c[i] - beta_c[j]) * (E[i] - E[j]), np.nan)
    free = finite & (d >= 0.0)
    drew = finite & ~free
    with np.errstate(invalid="ignore", over="ignore"):  # exp(d) of the pairs that did not draw is not used
        accept = free | (drew & (u[i] < np.exp(d)))
    a, b = i[accept], j[accept]
    for k in SWAPPED:
        if k in arrays:
            v = arrays[k]
            tmp = v[a].copy()
            v[a] = v[b]
            v[b] = tmp
    if swap_attempts is not None:
        swap_attempts[i] += 1
    if swap_accepts is not None:
        swap_accepts[a] += 1
    return i, accept, drew, d


def trip_bookkeeping(R, T, parity, replica_id, trip_dir, round_trips):
    """After a round's exchanges, in place.  trip_dir / round_trips are indexed r T + label.
    A pair holding rung 0 (parity 0 only): the label now at rung 0 counts a round trip if its
    trip_dir is 2, then its trip_dir is 1.  A pair holding rung T - 1: the label now there
    turns a trip_dir of 1 into 2.  (Rung 0 first: with T = 2 one pair holds both.)"""
    base = np.arange(R) * T
    if parity == 0:
        k = base + replica_id[base]
        round_trips[k] += trip_dir[k] == 2
        trip_dir[k] = 1
    if (T - 2 - parity) % 2 == 0 and T - 2 >= parity:  # rung T - 2 is a pair's lower rung
        k = base + replica_id[base + T - 1]
        trip_dir[k] = np.where(trip_dir[k] == 1, 2, trip_dir[k])


def initial_bookkeeping(R, T):
    """(replica_id int32, trip_dir int8, round_trips int64) as the engine starts them."""
    t = np.tile(np.arange(T), R)
    return t.astype(np.int32), (t == 0).astype(np.int8), np.zeros(R * T, np.int64)


# ---------------------------------------------------------------- the N = 1 system
def well_energy(x, y, box=BOX, v0=V0, r0=R0, k=K):
    """The double well of one particle: wells at (box/4, box/2) and (3 box/4, box/2), each
    v0_i (1 - (1 + tanh(k (r - r0))) / 2) with the minimum-image distance r to its centre."""
    v = np.zeros_like(np.asarray(x, dtype=np.float64))
    for cx, depth in ((box / 4.0, v0[0]), (3.0 * box / 4.0, v0[1])):
        dx, dy = x - cx, y - box / 2.0
        dx = dx - box * np.round(dx / box)
        dy = dy - box * np.round(dy / box)
        r = np.sqrt(dx * dx + dy * dy)
        v = v + depth * (1.0 - 0.5 * (1.0 + np.tanh(k * (r - r0))))
    return v


def p_left_exact(temperature, n=2000):
    """P(x < box / 2) = Z(x < box / 2) / Z of one particle at `temperature`, midpoint rule on
    an n x n grid over the box."""
    g = (np.arange(n) + 0.5) * (BOX / n)
    w = np.exp(-well_energy(g[:, None], g[None, :]) / temperature)
    return float(w[g < BOX / 2.0].sum() / w.sum())


def sample_ladders(R, rounds, moves_per_round, seed, temperatures=EXACT_TEMPERATURES, exchange=True):
    """R ladders of the N = 1 system from EXACT_START: per round moves_per_round local moves
    (the engine's rule: each coordinate displaced by (u - 0.5) max_disp, wrapped with np.mod;
    a lower or equal energy accepts, else u < exp(-beta dE)) then one exchange round of
    alternating parity.  Returns (x [R][T] of the final snapshot, exchange rates [T - 1])."""
    rng = np.random.default_rng(seed)
    T = len(temperatures)
    C = R * T
    beta_c = np.tile(1.0 / np.asarray(temperatures, dtype=np.float64), R)
    xy = np.tile(np.asarray(EXACT_START, dtype=np.float64), (C, 1))
    E = well_energy(xy[:, 0], xy[:, 1])
    att, acc = np.zeros(C, np.int64), np.zeros(C, np.int64)
    for rnd in range(rounds):
        for _ in range(moves_per_round):
            new = np.mod(xy + (rng.random((C, 2)) - 0.5) * EXACT_MAX_DISP, BOX)
            en = well_energy(new[:, 0], new[:, 1])
            ok = (en <= E) | (rng.random(C) < np.exp(np.minimum(0.0, -beta_c * (en - E))))
            xy[ok] = new[ok]
            E[ok] = en[ok]
        if exchange:
            arrays = {"state": xy, "E": E}
            exchange_round(R, T, rnd % 2, beta_c, arrays, rng.random(C), att, acc)
    a, b = att.reshape(R, T).sum(0)[:T - 1], acc.reshape(R, T).sum(0)[:T - 1]
    return xy[:, 0].reshape(R, T), b / np.maximum(a, 1)
