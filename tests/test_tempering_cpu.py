"""CPU checks of the temperature-ladder feature: the argument checks of its four C entry
points (no device: validation fails before any launch), their declarations and bindings, the
ladder layout and its validation, and the numpy statement of the exactness system
(tempering_cases.py) against quadrature."""
import ctypes
import json
import os

import numpy as np
import pytest

from flowstate import _lib, io
from flowstate.MCMC import Physics, TemperedMonteCarlo
from flowstate.MCMC.tempered import ladder_layout
from tempering_cases import (EXACT_TEMPERATURES, exchange_round, initial_bookkeeping, p_left_exact, sample_ladders,
                             trip_bookkeeping)
from test_host_cpu import header_symbols

NEW = ("fs_local_moves_beta", "fs_mh_accept_beta", "fs_nf_mh_step_beta", "fs_replica_exchange")
P_LEFT = (0.1213, 0.2535, 0.3758, 0.4632)  # quadrature values at EXACT_TEMPERATURES


def test_new_entry_points_are_declared_exported_and_bound():
    L = _lib.load()
    syms = header_symbols()
    for name in NEW:
        assert name in syms, f"{name} not declared in include/flowstate.h"
        assert hasattr(L, name), f"{name} not exported"
        assert name in _lib.EXPORTED, f"{name} not bound in flowstate._lib"


def test_beta_entry_points_check_their_arguments_like_their_siblings():
    L = _lib.load()
    ph = _lib.Phys()
    one = ctypes.c_void_p(1)  # never dereferenced: validation fails first
    rc = L.fs_local_moves_beta(one, ph, 4, 65, one, None, one, None, one, one, one, one, one, None, 10, 0, 0, 0.5, 0,
                               None, None, None, None, None, None)
    assert rc == -1 and b"fs_local_moves_beta: N=65" in L.fs_last_error()
    rc = L.fs_local_moves_beta(None, ph, 4, 16, one, None, one, None, one, one, one, one, one, None, 10, 0, 50, 0.5, 0,
                               None, None, None, None, None, None)
    assert rc == -1 and b"fs_local_moves_beta: adjust_every" in L.fs_last_error()
    rc = L.fs_local_moves_beta(one, ph, 4, 16, one, None, one, None, one, one, one, one, one, None, 10, 0, 0, 0.5, 5,
                               None, None, None, None, one, None)
    assert rc == -1 and b"sample_every" in L.fs_last_error()
    rc = L.fs_local_moves_beta(one, ph, 4, 16, None, None, one, None, one, one, one, one, one, None, 10, 0, 0, 0.5, 0,
                               None, None, None, None, None, None)
    assert rc == -1 and b"fs_local_moves_beta: invalid arguments" in L.fs_last_error()
    # the plain entry points keep their messages
    rc = L.fs_local_moves(ph, 4, 65, one, None, one, None, one, one, one, one, one, None, 10, 0, 0, 0.5, 0, None,
                          None, None, None, None)
    assert rc == -1 and b"fs_local_moves: N=65" in L.fs_last_error()
    rc = L.fs_mh_accept_beta(one, ph, 4, 0, one, None, one, one, None, one, one, None, None, None, one, None, None,
                             None, 0, None)
    assert rc == -1 and b"fs_mh_accept_beta: N=0" in L.fs_last_error()
    rc = L.fs_mh_accept_beta(one, ph, 4, 3, one, None, one, one, None, one, one, one, None, None, one, None, None,
                             None, 0, None)
    assert rc == -1 and b"state and config go together" in L.fs_last_error()
    rc = L.fs_mh_accept_beta(one, None, 4, 3, one, None, one, one, None, one, one, None, None, None, one, None, None,
                             None, 0, None)
    assert rc == -1 and b"fs_mh_accept_beta: invalid arguments" in L.fs_last_error()
    d64 = _lib.FlowDims(N=16, L=2, H=64, nb=1, K=8, precision=0, tail_bound=5.0)
    rc = L.fs_nf_mh_step_beta(one, d64, one, ph, 4, 0, 0, 0, None, None, None, None, None, None, None, None, None,
                              None, None, 0, one, None)
    assert rc == -1 and b"fs_nf_mh_step_beta" in L.fs_last_error()
    aligned = ctypes.c_void_p(256)
    rc = L.fs_nf_mh_step_beta(one, d64, one, ph, 4, 0, 0, 0, one, one, one, one, None, None, one, None, None, None,
                              None, _lib.FS_MH_HYBRID, aligned, None)
    assert rc == -1 and b"FS_MH_HYBRID needs the state" in L.fs_last_error()
    rc = L.fs_nf_mh_step_beta(one, d64, one, ph, 4, 0, 0, 0, one, one, one, one, None, None, one, None, None, None,
                              None, 0, one, None)
    assert rc == -1 and b"aligned" in L.fs_last_error()
    bad = _lib.FlowDims(N=16, L=2, H=96, nb=1, K=8, precision=0, tail_bound=5.0)
    rc = L.fs_nf_mh_step_beta(one, bad, one, ph, 4, 0, 0, 0, one, one, one, one, None, None, one, None, None, None,
                              None, 0, aligned, None)
    assert rc == _lib.FS_EUNSUPPORTED and b"H=96" in L.fs_last_error()


def test_replica_exchange_names_the_bad_argument():
    L = _lib.load()
    ok = ctypes.c_void_p(256)

    def call(R=4, T=4, N=3, parity=0, beta=ok, state=ok, E=ok, pcg=ok, rid=None, trip=None, trips=None):
        return L.fs_replica_exchange(R, T, N, parity, beta, state, None, E, None, None, pcg, rid, None, None, trip,
                                     trips, None)

    for kw, word in ((dict(T=1), b"T=1"), (dict(parity=2), b"parity=2"), (dict(parity=-1), b"parity=-1"),
                     (dict(N=0), b"N=0"), (dict(N=65), b"N=65"), (dict(beta=None), b"beta_c"),
                     (dict(state=None), b"state"), (dict(E=None), b"E is NULL"), (dict(pcg=None), b"pcg"),
                     (dict(state=ctypes.c_void_p(8)), b"16-byte"), (dict(R=-1), b"R=-1"),
                     (dict(trip=ok), b"replica_id"), (dict(rid=ok, trips=ok), b"trip_dir")):
        assert call(**kw) == -1, kw
        msg = L.fs_last_error()
        assert msg.startswith(b"fs_replica_exchange") and word in msg, (kw, msg)
    assert call(R=0) == 0  # nothing to do, nothing launched


def test_ladder_layout_and_validation():
    R, T, temps, beta, index = ladder_layout(12, (0.7, 1.0, 1.5, 2.3))
    assert (R, T) == (3, 4)
    np.testing.assert_array_equal(index, np.tile(np.arange(4), 3))
    np.testing.assert_array_equal(beta, np.tile(1.0 / np.array([0.7, 1.0, 1.5, 2.3]), 3))
    assert beta.dtype == np.float64 and temps.dtype == np.float64
    for C, temps in ((12, (1.0, 1.0, 2.0)), (12, (2.0, 1.0, 3.0)), (12, (1.0,)), (10, (1.0, 2.0, 3.0, 4.0)),
                     (12, (0.0, 1.0, 2.0)), (12, (1.0, 2.0, float("nan"))), (0, (1.0, 2.0))):
        with pytest.raises(ValueError):
            ladder_layout(C, temps)
    # the engine refuses a bad ladder before it needs a device
    xy = np.zeros((10, 3, 2))
    for temps in ((1.0, 1.0), (1.0,), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError):
            TemperedMonteCarlo(None, xy, Physics(8.0, 8.0), np.arange(10, dtype=np.uint64), temps)


def test_exchange_statement_on_a_small_case():
    """The numpy statement itself on hand-checked pairs: an infinite energy rejects without a
    draw, d >= 0 accepts without one, d < 0 compares the draw with exp(d)."""
    T, R = 4, 1
    beta = 1.0 / np.array([1.0, 2.0, 4.0, 8.0])
    E = np.array([3.0, 1.0, 2.0, 5.0])  # pair (0, 1): d = 0.5 * 2 = 1 >= 0; pair (2, 3): d = 0.125 * -3 < 0
    arrays = {"E": E.copy(), "replica_id": np.arange(4, dtype=np.int32)}
    u = np.array([0.99, 0.0, np.exp(-0.375) - 1e-9, 0.0])
    att, acc = np.zeros(4, np.int64), np.zeros(4, np.int64)
    i, accept, drew, d = exchange_round(R, T, 0, beta, arrays, u, att, acc)
    assert i.tolist() == [0, 2] and accept.tolist() == [True, True] and drew.tolist() == [False, True]
    assert arrays["E"].tolist() == [1.0, 3.0, 5.0, 2.0] and arrays["replica_id"].tolist() == [1, 0, 3, 2]
    assert att.tolist() == [1, 0, 1, 0] and acc.tolist() == [1, 0, 1, 0]
    arrays = {"E": np.array([np.inf, 1.0, 2.0, 5.0])}
    u[2] = np.exp(-0.375)  # not below exp(d): reject
    i, accept, drew, d = exchange_round(R, T, 0, beta, arrays, u)
    assert accept.tolist() == [False, False] and drew.tolist() == [False, True]
    i, accept, drew, d = exchange_round(R, T, 1, beta, arrays, u)
    assert i.tolist() == [1]


def test_round_trip_statement_follows_the_odd_even_transposition():
    """With every exchange accepted the labels follow the odd-even transposition sort: label 0
    reaches the top after T rounds and is back after 2 T, which counts one round trip."""
    for T in (2, 3, 4, 5):
        rid, trip, trips = initial_bookkeeping(2, T)
        beta = np.ones(2 * T)
        for rnd in range(4 * T):
            arrays = {"E": np.zeros(2 * T), "replica_id": rid}
            exchange_round(2, T, rnd % 2, beta, arrays, np.ones(2 * T))
            trip_bookkeeping(2, T, rnd % 2, rid, trip, trips)
            assert sorted(rid[:T].tolist()) == list(range(T))
        assert trips.sum() > 0 and trips[0] == trips[T]
        assert trips[0] >= 1


def test_write_tempering(tmp_path):
    summary = {"R": 1, "T": 2, "pairs": [{"rungs": [0, 1], "attempts": 3, "accepts": 1, "rate": 1 / 3}],
               "round_trips": {"per_ladder": [0], "total": 0}, "temperatures": []}
    path = io.write_tempering(str(tmp_path), summary)
    assert os.path.basename(path) == "tempering_data.json"
    assert json.load(open(path)) == summary


def test_quadrature_values():
    for T, want in zip(EXACT_TEMPERATURES, P_LEFT):
        assert abs(p_left_exact(T, n=1000) - want) < 5e-4


@pytest.mark.slow
def test_numpy_sampler_matches_quadrature():
    """R = 1024 ladders, 400 rounds of 50 moves and one exchange: each temperature's final
    P_left within 5 binomial standard deviations of the quadrature value."""
    R = 1024
    x, rates = sample_ladders(R, 400, 50, seed=1)
    for t, T in enumerate(EXACT_TEMPERATURES):
        p = p_left_exact(T)
        got = float((x[:, t] < 4.0).mean())
        print(f"T={T}: P_left {got:.4f} exact {p:.4f} bound {5 * np.sqrt(p * (1 - p) / R):.4f}")
        assert abs(got - p) <= 5.0 * np.sqrt(p * (1.0 - p) / R)
    print("exchange rates", rates)
