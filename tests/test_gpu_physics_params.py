"""The Monte-Carlo physics kernels (physics_kernels.hip, physics_device.h, local_kernels.hip)
away from the drivers' square box, two wells, default V0 / r0 / k and beta = 1: parameter
sets P1-P3 of physics_params_cases.py (aspect 1.6 / 0.55, V0 = (-4, 3), r0 = 0.8, k = 7, two /
one / no wells), temperatures 0.6 and 3, beta 0.37 and 2.5, against the C oracle (pinned to
the reference at these parameters by tests/test_oracle_params.py) with the tolerances of the
square-box tests: 1e-12 on energies and virials; flags, masks, states and RNG state bit-exact."""
import os

import numpy as np
import pytest
import torch

import physics_params_cases as PC
from flowstate.MCMC import BatchedMonteCarlo, EnergyCalculator, SimulationBox
from flowstate.MCMC.energy_calculator import total_energy
from oracle import physics as OP

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _close(a, b):
    return (np.isinf(a) and np.isinf(b) and a == b) or abs(a - b) <= 1e-12 * max(1.0, abs(b))


def _masks(nbr, N):
    words = nbr.cpu().numpy().view(np.uint64)
    return ((words[:, :, None] >> np.arange(N, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [3, 16, 33])
@pytest.mark.parametrize("name", ["P1", "P2", "P3"])
def test_total_energy_on_rectangular_boxes(name, N, dtype):
    """fs_energy_lj_dw with Lx != Ly and other well constants, 257 chains (an odd count: the
    last wave half is empty): rows whose only in-cutoff pair crosses the y edge, rows where it
    crosses the x edge, particles inside the wells, hard-core overlaps."""
    C = 257
    ph = PC.oracle_phys(N, name)
    pos = PC.positions(N, C, name, dtype)
    finite_wrap = PC.check_wrap_rows(pos, ph)
    Eo, Wo, ovo = OP.total_energy_batch(pos, ph)
    E, W, ov, nbr = total_energy(torch.from_numpy(pos).cuda(), PC.device_phys(N, name), with_neighbours=True)
    E, W, ov = E.cpu().numpy(), W.cpu().numpy(), ov.cpu().numpy()
    np.testing.assert_array_equal(ov, ovo)
    fin = np.isfinite(Eo)
    assert np.array_equal(np.isfinite(E), fin) and np.array_equal(np.isfinite(W), fin)
    np.testing.assert_allclose(E[fin], Eo[fin], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(W[fin], Wo[fin], rtol=1e-12, atol=1e-12)
    assert 0 < fin.sum() < C and fin[finite_wrap].all()
    got = _masks(nbr, N)
    for c in finite_wrap + [PC.SPECIAL - 1, PC.SPECIAL + 1, C - 1]:
        if not fin[c]:
            continue
        _, _, _, cut = OP.total_energy(pos[c], ph, with_cutoff=True)
        np.testing.assert_array_equal(got[c], np.triu(cut, 1), err_msg=f"chain {c}")
    assert all(got[c][0, 1] for c in finite_wrap)
    # a second launch without the masks gives the same numbers
    E2, W2, ov2 = total_energy(torch.from_numpy(pos).cuda(), PC.device_phys(N, name))
    np.testing.assert_array_equal(E2.cpu().numpy(), E)
    np.testing.assert_array_equal(W2.cpu().numpy(), W)


@pytest.mark.parametrize("N", [3, 16, 33])
def test_energy_state_mixed_dtypes_on_a_rectangular_box(N):
    """fs_energy_state (float64 storage, per-chain dtype flags) at P1: each chain's energy is
    the oracle's in that chain's own dtype."""
    C = 257
    ph = PC.oracle_phys(N, "P1")
    pos = PC.positions(N, C, "P1", np.float64, seed=5)
    f32 = np.random.default_rng(N).random(C) < 0.5
    state = np.where(f32[:, None, None], pos.astype(np.float32).astype(np.float64), pos)
    b = BatchedMonteCarlo(None, state, PC.device_physics(N, "P1"), np.arange(C, dtype=np.uint64))
    b.state_is_f32.copy_(torch.from_numpy(f32.astype(np.uint8)))
    E, W = (t.cpu().numpy() for t in b._energy_of_state())
    n32 = 0
    for c in range(C):
        x = state[c].astype(np.float32) if f32[c] else state[c]
        Eo, Wo, _ = OP.total_energy(x, ph)
        assert _close(E[c], Eo) and _close(W[c], Wo), (c, E[c], Eo)
        E_other = OP.total_energy(state[c] if f32[c] else state[c].astype(np.float32), ph)[0]
        n32 += bool(np.isfinite(Eo) and E_other != Eo and not _close(E[c], E_other))
    assert n32 >= 30  # the dtype flag matters: the other dtype's energy is outside the tolerance


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N", [3, 16])
@pytest.mark.parametrize("name", ["P1", "P2"])
def test_dropin_box_and_particle_energy_on_rectangular_boxes(name, N, dt):
    """SimulationBox.minimum_image / compute_distances (fs_min_image) and
    EnergyCalculator.calculate_particle_energy_virial (fs_particle_energy) with Lx != Ly, one
    or two wells: against the oracle on every pair / particle and against the reference's own
    outputs (tests/golden/physics_params.npz)."""
    f = np.load(os.path.join(G, "physics_params.npz"))
    tag = f"{name}_N{N}_{dt}"
    prm, ph = PC.PARAMS[name], PC.oracle_phys(N, name)
    box = SimulationBox(ph.Lx, ph.Ly)
    pos = f[tag + "_pos"]
    for c, x in enumerate(pos):
        for (i, j), want in zip(f[tag + "_ij"], f[tag + "_delta"][c]):
            d = box.minimum_image(x[i], x[j])
            assert d.dtype == x.dtype
            np.testing.assert_array_equal(d, want)
            np.testing.assert_array_equal(d, OP.min_image(x[i], x[j], ph))
        rows = box.compute_distances(x[0], x[1:])
        want = [np.linalg.norm(OP.min_image(x[0], q, ph)) for q in x[1:]]
        np.testing.assert_array_equal(rows, np.asarray(want, np.float64))
        ec = EnergyCalculator(N, x, box, num_wells=prm["num_wells"], V0_list=list(prm["V0"]), r0=prm["r0"],
                              k=prm["k"])
        Er, Wr = f[tag + "_EW"][c]
        assert _close(ec.total_energy, Er) and _close(ec.total_virial, Wr)
        for p in range(N):
            E, W = ec.calculate_particle_energy_virial(x, p)
            Eo, Wo = OP.particle_energy(x, p, ph)
            Er, Wr = f[tag + "_particle_ew"][c, p]
            assert _close(E, Eo) and _close(W, Wo), (c, p, E, Eo)
            assert _close(E, Er) and _close(W, Wr), (c, p, E, Er)


@pytest.mark.parametrize("N,C,moves,name,T", [(3, 32, 300, "P1", 0.6), (16, 32, 200, "P1", 0.6),
                                             (3, 32, 300, "P2", 3.0), (16, 32, 200, "P2", 3.0)])
def test_local_moves_at_other_boxes_and_temperatures(N, C, moves, name, T):
    """fs_local_moves with Lx != Ly (the move's wrap, the y minimum image, the well centres)
    and beta != 1 (the accept rule): every field of test_local_moves_match_oracle."""
    from test_gpu_local import check_local_moves

    ph = PC.oracle_phys(N, name)
    init = PC.cluster_positions(N, C, name)
    f32 = np.random.default_rng(N + 1).random(C) < 0.5
    log = check_local_moves(init, f32, moves, PC.device_physics(N, name, temperature=T), ph, 1.0 / T)
    assert 0.05 < log.mean() < 0.95
    # the temperature decides moves: the same chains at beta = 1 take other paths
    for c in range(4):
        other = OP.LocalChain(init[c].astype(np.float32) if f32[c] else init[c], 1000 + c, ph, max_disp=0.65)
        assert not np.array_equal(other.local_moves(moves, adjust_every=50).astype(np.uint8), log[c])


@pytest.mark.parametrize("beta", [0.37, 2.5])
@pytest.mark.parametrize("correct_sign", [False, True])
def test_accept_mask_at_other_temperatures(correct_sign, beta):
    """fs_mh_accept at beta != 1: masks and PCG64 states bit-exact, accepts and rejects both
    present, and the verdicts are not those of beta = 1."""
    from test_gpu_physics import accept_inputs, check_accept_mask

    acc = check_accept_mask(correct_sign, beta)
    assert 0 < acc.sum() < len(acc)
    E_old, E_new, nll_old, lq_new, seeds = accept_inputs()
    C = len(seeds)
    pcg = OP.pcg64_seed_many(seeds)
    one, _ = OP.mh_accept(E_old, E_new, nll_old, -lq_new.astype(np.float64), pcg, correct_sign=correct_sign)
    assert (one != acc).sum() > C // 50


@pytest.mark.parametrize("beta", [0.37, 2.5])
def test_bulk_judge_at_other_temperatures(beta):
    """fs_metropolis_judge at beta != 1 through the batched judges."""
    from test_gpu_judge import check_bulk_judge

    acc = check_bulk_judge(beta)
    assert 0 < acc.sum() < acc.size and (acc.sum(1) > 0).any() and (acc.sum(1) < acc.shape[1]).any()


def test_well_stats_at_another_radius():
    """fs_well_stats takes one half_box (square boxes only); r0 = 0.8 instead of the drivers'
    1.2, the particles spread in proportion, against the oracle's classify."""
    from test_gpu_physics import check_well_stats

    check_well_stats(1.0, 0.8, spread=0.4)
