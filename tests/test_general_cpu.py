"""Host-side checks of the general-shape flow mode (no GPU): fs_flow_dims.precision 4
("f32-general") sizes an image for any H <= 512, K <= 32, rejects values outside its range
with the value named, leaves the default mode's refusals as they are, and the runtime-K
training spline checks its arguments before touching the device."""
import pytest
import torch

from flowstate import _lib
from flowstate.models import build_flow
from flowstate.normflows.flows import PRECISIONS

# (N, L, H, nb, K): the shapes of tests/test_gpu_general.py
SHAPES = [(3, 2, 24, 1, 7), (3, 3, 40, 0, 10), (15, 2, 96, 2, 16), (4, 2, 48, 3, 1), (64, 2, 100, 1, 20),
          (64, 1, 320, 1, 31), (64, 2, 512, 1, 32)]


def test_general_mode_is_registered():
    assert PRECISIONS["f32-general"] == 4
    m = build_flow(4, 1, 32, 1, 5).set_precision("f32-general")
    assert m.precision == "f32-general" and m.dims().precision == 4
    assert m.set_precision("f32").dims().precision == 0


@pytest.mark.parametrize("N,L,H,nb,K", SHAPES)
def test_general_mode_sizes_any_shape(N, L, H, nb, K):
    m = build_flow(N, L, H, nb, K).set_precision("f32-general")
    lib = _lib.load()
    n_mod = sum(t.numel() for f in m.flows for t in f.raw_param_tensors())
    assert lib.fs_flow_raw_floats(m.dims()) == n_mod, lib.fs_last_error()
    nbytes = lib.fs_flow_packed_bytes(m.dims())
    assert nbytes > 0, lib.fs_last_error()
    # the image holds at least every GEMM weight once (H is only ever padded up)
    assert nbytes >= 4 * L * (2 * N * H + 2 * nb * H * H + N * (3 * K + 1) * H)


@pytest.mark.parametrize("field,value,text", [("H", 513, b"H=513"), ("K", 33, b"K=33"), ("N", 65, b"N=65"),
                                              ("H", 0, b"H=0"), ("K", 0, b"K=0")])
def test_general_mode_names_the_value_out_of_range(field, value, text):
    lib = _lib.load()
    d = build_flow(16, 1, 96, 1, 8).set_precision("f32-general").dims()
    assert lib.fs_flow_packed_bytes(d) > 0
    setattr(d, field, value)
    assert lib.fs_flow_packed_bytes(d) == -1 and text in lib.fs_last_error()
    assert lib.fs_flow_raw_floats(d) == -1 and text in lib.fs_last_error()
    # the device entry points refuse the same dims before they look at a buffer
    assert lib.fs_flow_pack(d, None, None, None) == -2 and text in lib.fs_last_error()
    assert lib.fs_flow_log_prob(d, None, None, 4, None, None, None, None) == -2


def test_mh_workspace_sizes_accept_general_dims():
    """The fused MH step, the multi-step launch and the proposal bank size their workspaces
    for a general-mode flow (they refuse the same dims in the default mode)."""
    lib = _lib.load()
    m = build_flow(16, 3, 96, 1, 10)
    d0, d3 = m.dims(), m.set_precision("f32-general").dims()
    for fn, extra in ((lib.fs_nf_mh_step_ws_bytes, ()), (lib.fs_nf_mh_steps_ws_bytes, (4,)),
                      (lib.fs_nf_mh_banked_ws_bytes, ())):
        assert fn(d3, 512, *extra) > 0, lib.fs_last_error()
        assert fn(d0, 512, *extra) == -1


def test_default_mode_still_refuses_uninstantiated_shapes():
    lib = _lib.load()
    d = build_flow(16, 1, 96, 1, 8).dims()
    assert d.precision == 0
    assert lib.fs_flow_raw_floats(d) == -1
    err = lib.fs_last_error()
    assert b"unsupported" in err and b"H=96" in err and b"f32-general" in err
    for prec in (1, 2):  # the split modes do not gain the general shapes
        d.precision = prec
        assert lib.fs_flow_packed_bytes(d) == -1


def test_runtime_k_spline_rejects_invalid_arguments_before_touching_the_device():
    lib = _lib.load()
    one = torch.zeros(64)
    p = _lib.ptr(one)  # a host address: never dereferenced by a refused call
    assert lib.fs_rqs_forward_any(1, 33, 0, p, p, p, p, 3.0, p, p, None, None) == -1
    assert b"K=33" in lib.fs_last_error()
    assert lib.fs_rqs_forward_any(1, 0, 0, p, p, p, p, 3.0, p, p, None, None) == -1
    assert lib.fs_rqs_forward_any(1, 10, 0, None, p, p, p, 3.0, p, p, None, None) == -1
    assert lib.fs_rqs_forward_any(1, 10, 0, p, p, p, p, 3.0, None, p, None, None) == -1
    assert lib.fs_rqs_forward_any(1, 10, 0, p, p, p, p, 0.0, p, p, None, None) == -1
    assert lib.fs_rqs_backward_any(1, 33, 0, p, p, p, p, 3.0, None, None, p, p, p, p, None) == -1
    assert b"K=33" in lib.fs_last_error()
    assert lib.fs_rqs_backward_any(1, 10, 0, p, p, p, p, 3.0, None, None, None, p, p, p, None) == -1
    # the instantiated entry points keep their own list
    assert lib.fs_rqs_forward(1, 10, 0, p, p, p, p, 3.0, p, p, None, None) == -1
    assert b"K=10" in lib.fs_last_error()
    # nothing to do: accepted without a launch
    assert lib.fs_rqs_forward_any(0, 10, 0, None, None, None, None, 3.0, None, None, None, None) == 0


def test_device_spline_keeps_raising_without_any_k():
    from flowstate.normflows import autograd_flow as AF

    class FakeDevice:  # stands for a device tensor (no GPU here): only is_cuda is read
        is_cuda = True

    uw, ud = torch.zeros(4, 10), torch.zeros(4, 11)
    with pytest.raises(_lib.FlowStateError, match="K=10"):
        AF.circular_rqs(FakeDevice(), uw, uw, ud, 3.0, False, any_k=False)
    with pytest.raises(_lib.FlowStateError, match="K=33"):  # past the runtime-K kernels' range
        AF.circular_rqs(FakeDevice(), torch.zeros(4, 33), torch.zeros(4, 33), torch.zeros(4, 34), 3.0, False,
                        any_k=True)
    x = torch.linspace(-2.0, 2.0, 4)  # CPU tensors: the torch restatement either way
    a = AF.circular_rqs(x, uw, uw, ud, 3.0, False, any_k=True)
    b = AF.circular_rqs(x, uw, uw, ud, 3.0, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
