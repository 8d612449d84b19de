"""fs_coupling.any_k on the host side (no GPU): the descriptor keeps its 48 bytes, and
check_coupling accepts 1 <= K <= 32 with any_k set, keeps refusing uninstantiated bin counts
without it, and refuses descriptors of one call that disagree on it.  rows = 0 everywhere:
validation runs, nothing launches and no pointer is read."""
import ctypes

import pytest

from flowstate import _lib

ONE, TWO = ctypes.c_void_p(1), ctypes.c_void_p(2)  # never dereferenced (rows = 0)


def desc(K, any_k, rows=0):
    return _lib.Coupling(rows=rows, D=16, K=K, hidden=64, any_k=any_k, identity_features=1, transform_features=1,
                         tail_bound=3.0)


def density_fwd(c):
    return _lib.load().fs_coupling_density_fwd(ctypes.byref(c), ONE, ONE, ONE, ONE, ONE, None, TWO, ONE, None)


def sample_pre(c):
    return _lib.load().fs_coupling_sample_pre(ctypes.byref(c), ONE, ONE, ONE, ONE, ONE, TWO, ONE, None, None)


def test_coupling_descriptor_layout():
    assert ctypes.sizeof(_lib.Coupling) == 48
    assert _lib.Coupling.any_k.offset == 20 and _lib.Coupling.identity_features.offset == 24
    c = _lib.Coupling(rows=4, D=16, K=8, hidden=64, identity_features=1, transform_features=1, tail_bound=3.0)
    assert c.any_k == 0


@pytest.mark.parametrize("K", [1, 7, 10, 32])
def test_any_k_accepts_every_bin_count_up_to_32(K):
    assert density_fwd(desc(K, 1)) == 0
    assert sample_pre(desc(K, 1)) == 0


@pytest.mark.parametrize("K", [0, 33])
def test_any_k_refuses_bin_counts_outside_the_range(K):
    L = _lib.load()
    for call in (density_fwd, sample_pre):
        assert call(desc(K, 1)) == -1
        assert f"K={K}".encode() in L.fs_last_error()


def test_without_any_k_uninstantiated_bin_counts_still_fail():
    L = _lib.load()
    for call in (density_fwd, sample_pre):
        assert call(desc(7, 0)) == -1
        assert b"K=7 not instantiated" in L.fs_last_error()
    assert density_fwd(desc(8, 0)) == 0


def test_descriptors_of_one_call_must_agree_on_any_k():
    L = _lib.load()
    for ks, kd in ((1, 0), (0, 1)):
        s, d = desc(8, ks), desc(8, kd)
        rc = L.fs_coupling_pair_pre(ctypes.byref(s), ONE, ONE, ONE, ONE, ONE, TWO, ONE, None, ctypes.byref(d), ONE, ONE,
                                    None)
        assert rc == -1 and b"any_k" in L.fs_last_error()
    s, d = desc(10, 1), desc(10, 1)
    assert L.fs_coupling_pair_pre(ctypes.byref(s), ONE, ONE, ONE, ONE, ONE, TWO, ONE, None, ctypes.byref(d), ONE, ONE,
                                  None) == 0
    # bwd_step and pair_step likewise; with any_k they also need one K
    f, c = desc(10, 1), desc(10, 0)
    rc = L.fs_coupling_bwd_step(ctypes.byref(f), ONE, ONE, ONE, None, ctypes.byref(c), ONE, ONE, ONE, ONE, ONE, None, ONE,
                                ONE, ONE, None)
    assert rc == -1  # c: K=10 without any_k
    f, c = desc(8, 1), desc(8, 0)
    rc = L.fs_coupling_bwd_step(ctypes.byref(f), ONE, ONE, ONE, None, ctypes.byref(c), ONE, ONE, ONE, ONE, ONE, None, ONE,
                                ONE, ONE, None)
    assert rc == -1 and b"any_k" in L.fs_last_error()
    f, c = desc(7, 1), desc(10, 1)
    rc = L.fs_coupling_bwd_step(ctypes.byref(f), ONE, ONE, ONE, None, ctypes.byref(c), ONE, ONE, ONE, ONE, ONE, None, ONE,
                                ONE, ONE, None)
    assert rc == -1 and b"any_k" in L.fs_last_error()
    f, c = desc(10, 1), desc(10, 1)
    assert L.fs_coupling_bwd_step(ctypes.byref(f), ONE, ONE, ONE, None, ctypes.byref(c), ONE, ONE, ONE, ONE, ONE, None,
                                  ONE, ONE, ONE, None) == 0
    s, d, s2, d2 = desc(10, 1), desc(10, 1), desc(10, 1), desc(10, 0)
    rc = L.fs_coupling_pair_step(ctypes.byref(s), ONE, ONE, None, ONE, ONE, None, ctypes.byref(s2), ONE, ONE, ONE, ONE, TWO,
                                 ONE, ctypes.byref(d), ONE, ONE, ONE, ONE, ONE, None, TWO, ONE, ctypes.byref(d2), ONE, None)
    assert rc == -1
    d2 = desc(8, 0)
    rc = L.fs_coupling_pair_step(ctypes.byref(s), ONE, ONE, None, ONE, ONE, None, ctypes.byref(s2), ONE, ONE, ONE, ONE, TWO,
                                 ONE, ctypes.byref(d), ONE, ONE, ONE, ONE, ONE, None, TWO, ONE, ctypes.byref(d2), ONE, None)
    assert rc == -1 and b"any_k" in L.fs_last_error()
    d2 = desc(10, 1)
    rc = L.fs_coupling_pair_step(ctypes.byref(s), ONE, ONE, None, ONE, ONE, None, ctypes.byref(s2), ONE, ONE, ONE, ONE, TWO,
                                 ONE, ctypes.byref(d), ONE, ONE, ONE, ONE, ONE, None, TWO, ONE, ctypes.byref(d2), ONE, None)
    assert rc == 0, L.fs_last_error()
