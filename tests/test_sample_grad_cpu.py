"""The sampling-direction backward on the host side (no GPU): the new entry points are
exported as include/flowstate.h declares them, fs_coupling_sample_bwd_* validate their
descriptors like every other coupling launch (rows = 0: validation runs, nothing launches
and no pointer is read), and CPU tensors keep the torch path."""
import ctypes
import os
import re

import pytest
import torch

from flowstate import _lib
from flowstate.normflows import autograd_flow as AF

ONE, TWO = ctypes.c_void_p(1), ctypes.c_void_p(2)  # never dereferenced (rows = 0)
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "flowstate.h")
NEW = ["fs_coupling_sample_bwd_post", "fs_coupling_sample_bwd_pre", "fs_coupling_sample_bwd_step", "fs_kld_loss_mix",
       "fs_kld_loss_mix_backward"]


def desc(K, any_k, D=16, rows=0):
    return _lib.Coupling(rows=rows, D=D, K=K, hidden=64, any_k=any_k, identity_features=1, transform_features=1,
                         tail_bound=3.0)


def bwd_post(c):
    return _lib.load().fs_coupling_sample_bwd_post(c and ctypes.byref(c), ONE, ONE, None, None, ONE, ONE, None)


def bwd_pre(c):
    return _lib.load().fs_coupling_sample_bwd_pre(c and ctypes.byref(c), ONE, ONE, ONE, ONE, ONE, ONE, None, None, ONE,
                                                  ONE, None)


def bwd_step(c, prev):
    return _lib.load().fs_coupling_sample_bwd_step(c and ctypes.byref(c), ONE, ONE, ONE, ONE, ONE, ONE, None, None, ONE,
                                                   ONE, prev and ctypes.byref(prev), ONE, ONE, None, TWO, ONE, None)


CALLS = [bwd_post, bwd_pre, lambda c: bwd_step(c, c)]


@pytest.mark.parametrize("name", NEW)
def test_new_symbols_are_declared_bound_and_exported(name):
    text = open(HEADER).read()
    m = re.search(r"\bint\s+%s\s*\(" % name, text)
    assert m, f"{name} is not declared in flowstate.h"
    # each declaration's comment cites the reference lines it restates
    comment = text[:m.start()].rsplit("/*", 1)[1]
    assert "core.py:105-142" in comment, name
    if "coupling" in name:
        assert "coupling.py:104-134" in comment, name
    assert getattr(_lib.load(), name).restype is ctypes.c_int


def test_null_descriptor_is_refused():
    L = _lib.load()
    for call in (bwd_post, bwd_pre):
        assert call(None) == -1
        assert b"invalid coupling description" in L.fs_last_error()
    assert bwd_step(None, desc(8, 0)) == -1 and b"invalid coupling description" in L.fs_last_error()
    assert bwd_step(desc(8, 0), None) == -1 and b"invalid coupling description" in L.fs_last_error()


@pytest.mark.parametrize("K", [0, 33])
def test_any_k_refuses_bin_counts_outside_the_range(K):
    L = _lib.load()
    for call in CALLS:
        assert call(desc(K, 1)) == -1
        assert f"K={K} outside 1..32".encode() in L.fs_last_error()


def test_without_any_k_uninstantiated_bin_counts_fail():
    L = _lib.load()
    for call in CALLS:
        assert call(desc(7, 0)) == -1
        assert b"K=7 not instantiated" in L.fs_last_error()


@pytest.mark.parametrize("K,any_k", [(5, 0), (8, 0), (15, 0), (32, 0), (1, 1), (10, 1), (32, 1)])
def test_valid_descriptors_pass(K, any_k):
    for call in CALLS:
        assert call(desc(K, any_k)) == 0, _lib.load().fs_last_error()


def test_step_needs_one_layer_shape():
    L = _lib.load()
    for c, prev in ((desc(8, 0), desc(5, 0)), (desc(8, 1), desc(8, 0)), (desc(8, 0), desc(8, 0, D=18)),
                    (desc(8, 0, D=258), desc(8, 0, D=258))):
        assert bwd_step(c, prev) == -1
        assert b"fs_coupling_sample_bwd_step: the layers differ" in L.fs_last_error()


def test_loss_head_refuses_empty_and_null_inputs():
    L = _lib.load()
    assert L.fs_kld_loss_mix(ONE, 0, ONE, ONE, 4, 0.5, None, ONE, None, None) == -1
    assert b"fs_kld_loss_mix: invalid arguments" in L.fs_last_error()
    assert L.fs_kld_loss_mix(ONE, 4, None, ONE, 4, 0.5, None, ONE, None, None) == -1
    assert L.fs_kld_loss_mix_backward(None, 4, 4, 0.5, ONE, ONE, ONE, None) == -1
    assert b"fs_kld_loss_mix_backward: invalid arguments" in L.fs_last_error()


def test_cpu_tensors_keep_the_torch_path():
    """reverse_kld with gradients on CPU tensors: no layer takes sample_step_grad, and the
    mixed loss of CPU vectors is the torch expression."""
    from test_train_cpu import build

    m, _ = build("cpu")
    before = AF.sample_grad_steps
    loss, _ = m.reverse_kld(8)
    loss.backward()
    assert AF.sample_grad_steps == before
    assert not AF._pending_sample_bwd
    lq, e, lr = torch.randn(5), torch.randn(7), torch.randn(7)
    for alpha in (0.0, 0.3):
        want = alpha * (-lq.mean()) + (1 - alpha) * (e.mean() + lr.mean())
        assert torch.equal(AF.kld_loss_mix(lq, e, lr, alpha), want)


def test_switch_follows_the_environment_and_defaults_on():
    assert AF._fused_sample_grad == (os.environ.get("FS_FUSED_SAMPLE_GRAD", "1") != "0")
    assert AF._sample_bwd_step is True
