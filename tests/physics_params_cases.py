"""Parameter sets and configurations shared by test_oracle_params.py, test_gpu_physics_params.py
and tests/golden/make_params_golden.py: the Monte-Carlo physics away from the drivers' square
box, two wells, default V0 / r0 / k and beta = 1."""
import numpy as np

from oracle import physics as OP

PARAMS = {
    "P1": dict(aspect=1.6, V0=(-4.0, 3.0), r0=0.8, k=7.0, num_wells=2),
    "P2": dict(aspect=0.55, V0=(-4.0, 3.0), r0=0.8, k=7.0, num_wells=1),
    "P3": dict(aspect=1.6, V0=(-4.0, 3.0), r0=0.8, k=7.0, num_wells=0),
}
N_YWRAP, N_XWRAP, N_WELL = 8, 8, 8   # the first rows of every batch, in this order
SPECIAL = N_YWRAP + N_XWRAP + N_WELL


def oracle_phys(N, name):
    return OP.make_phys(N, **PARAMS[name])


def device_phys(N, name, beta=1.0):
    """The library's fs_phys with the oracle's Lx, Ly."""
    from flowstate.MCMC.energy_calculator import make_phys

    p, o = PARAMS[name], oracle_phys(N, name)
    return make_phys(o.Lx, o.Ly, p["num_wells"], p["V0"], p["r0"], p["k"], beta)


def device_physics(N, name, temperature=1.0):
    """flowstate.MCMC.Physics with the oracle's Lx, Ly."""
    from flowstate.MCMC import Physics

    p, o = PARAMS[name], oracle_phys(N, name)
    return Physics(o.Lx, o.Ly, temperature=temperature, num_wells=p["num_wells"], V0_list=p["V0"], r0=p["r0"],
                   k=p["k"])


def positions(N, C, name, dtype, seed=0):
    """C configurations in [0, Lx) x [0, Ly): jittered lattices, every 7th uniform (every 14th with a sure
    hard-core overlap), and first
      N_YWRAP rows whose particles 0 and 1 are inside r_cut only through the y wrap,
      N_XWRAP rows whose particles 0 and 1 are inside r_cut only through the x wrap,
      N_WELL  rows with the last particle inside a well (alternating wells), near its edge."""
    ph = oracle_phys(N, name)
    Lx, Ly = ph.Lx, ph.Ly
    box = np.array([Lx, Ly])
    rng = np.random.default_rng(1000 * N + seed + sum(map(ord, name)))
    # a plain grid over the box (the reference's FCC start has coinciding sites at these aspects)
    nx = int(np.ceil(np.sqrt(N * Lx / Ly)))
    ny = int(np.ceil(N / nx))
    base = np.array([[(i + 0.5) * Lx / nx, (j + 0.5) * Ly / ny] for j in range(ny) for i in range(nx)])[:N]
    sigma = np.where(np.arange(C) < SPECIAL, 0.1, 0.35)[:, None, None]   # the special rows stay finite
    pos = np.mod(base[None] + sigma * rng.normal(0, 1, (C, N, 2)), box)
    pos[SPECIAL::7] = rng.random((len(pos[SPECIAL::7]), N, 2)) * box
    pos[SPECIAL::14, 1] = np.mod(pos[SPECIAL::14, 0] + [0.3, 0.1], box)   # a sure hard-core overlap (r < 0.5)

    def clear(c, placed):
        """No other particle within 0.8 (minimum image) of the placed ones: the row stays finite."""
        for q in placed:
            d = np.delete(pos[c], q, axis=0) - pos[c, q]
            d -= box * np.round(d / box)
            if np.min(np.hypot(d[:, 0], d[:, 1])) < 0.8:
                return False
        return True

    for c in range(min(C, SPECIAL)):
        for _ in range(200):
            if c < N_YWRAP:
                x0 = rng.uniform(1.0, Lx - 2.0)
                pos[c, 0] = [x0, rng.uniform(0.05, 0.5)]
                pos[c, 1] = [x0 + rng.uniform(-0.4, 0.4), Ly - rng.uniform(0.6, 1.2)]
                placed = (0, 1)
            elif c < N_YWRAP + N_XWRAP:
                y0 = rng.uniform(1.0, Ly - 2.0)
                pos[c, 0] = [rng.uniform(0.05, 0.5), y0]
                pos[c, 1] = [Lx - rng.uniform(0.6, 1.2), y0 + rng.uniform(-0.4, 0.4)]
                placed = (0, 1)
            else:
                cx = Lx / 4 if c % 2 == 0 else 3 * Lx / 4
                rad, ang = rng.uniform(0.3, 1.1), rng.uniform(0, 2 * np.pi)
                pos[c, N - 1] = np.mod([cx + rad * np.cos(ang), Ly / 2 + rad * np.sin(ang)], box)
                placed = (N - 1,)
            if clear(c, placed):
                break
    return np.ascontiguousarray(pos.astype(dtype))


def cluster_positions(N, C, name, seed=0):
    """C float64 configurations with all particles in one cluster at the LJ spacing (1.05 ..
    1.25), so that nearly every local move changes the energy by O(1) and the temperature
    decides it.  The clusters sit, in turn, on the first well, on the second well's place, across
    the box corner (both wraps act) and across the y = 0 edge."""
    ph = oracle_phys(N, name)
    box = np.array([ph.Lx, ph.Ly])
    rng = np.random.default_rng(77 * N + seed + sum(map(ord, name)))
    side = int(np.ceil(np.sqrt(N)))
    g = np.array([[i, j] for j in range(side) for i in range(side)], np.float64)[:N]
    g -= g.mean(axis=0)
    centres = np.array([[ph.Lx / 4, ph.Ly / 2], [3 * ph.Lx / 4, ph.Ly / 2], [0.0, 0.0], [ph.Lx / 2, 0.0]])
    pos = np.empty((C, N, 2))
    for c in range(C):
        pos[c] = centres[c % 4] + g * rng.uniform(1.05, 1.25) + rng.normal(0, 0.05, (N, 2))
    return np.mod(pos, box)


def check_wrap_rows(pos, ph):
    """On the oracle's side: the y-wrap and x-wrap rows hold a pair that is a neighbour only
    through that wrap, and some of those rows have a finite energy.  Returns the row indices
    with a finite energy."""
    finite = []
    for c in range(N_YWRAP + N_XWRAP):
        axis = 1 if c < N_YWRAP else 0
        d = pos[c, 0].astype(np.float64) - pos[c, 1].astype(np.float64)
        assert abs(d[axis]) > ph.r_cut and abs(d[1 - axis]) < 0.5          # apart without the wrap
        assert abs(d[axis]) > (ph.Ly if axis else ph.Lx) / 2                # and the wrap acts on that axis only
        r = OP.min_image_dist(pos[c], 0, 1, ph)
        assert ph.r_core < r <= ph.r_cut, (c, r)
        E, W, hit, cut = OP.total_energy(pos[c], ph, with_cutoff=True)
        assert cut[0, 1]
        if not hit:
            finite.append(c)
    assert sum(c < N_YWRAP for c in finite) >= 4 and sum(c >= N_YWRAP for c in finite) >= 4
    return finite
