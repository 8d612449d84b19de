"""Two builds of libflowstate.so give the same bits on the training splines' runtime-K kernels.

    tools/spline_family_bits.py compare LIB_A LIB_B [--out result.json]

Each build is loaded (FLOWSTATE_LIB) in processes of its own, which dump
  * out, lad, the NaN flag, gx, guw, guh, gud of fs_rqs_forward_any / fs_rqs_backward_any at K in
    {1, 7, 10, 31, 32}, both directions, M = 1000 (a ragged last workgroup), on the inputs of
    tests/test_gpu_general.py::_spline_case (values outside the bound, softplus above its threshold);
  * the loss and every parameter gradient of one general-mode paired step at
    (N=16, L=3, H=32, nb=1, K=10), 37 rows, once with FS_COUPLING_WAVES=0 and once with 1.
The arrays are compared with np.array_equal (NaNs equal); one JSON line says which are identical,
and the exit status is 1 unless all are.  `dump OUT.npz` is what the child processes run."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "flow-state_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SPLINE_K = (1, 7, 10, 31, 32)
STEP = (16, dict(L=3, H=32, nb=1, K=10), 37)


def spline_case(K, inverse, M):
    """_spline_case of tests/test_gpu_general.py."""
    import torch

    g = torch.Generator().manual_seed(K + 7 * int(inverse))
    B = 3.0
    x = (torch.rand(M, generator=g) * 2 - 1) * B * 1.05
    x[:4] = torch.tensor([B, -B, 0.0, B * 1.2])
    uw = torch.randn(M, K, generator=g) * 0.7
    uh = torch.randn(M, K, generator=g) * 0.7
    ud = torch.randn(M, K + 1, generator=g) * 0.7
    ud[:8, 0] = 25.0
    wo = torch.randn(M, generator=g)
    wl = torch.randn(M, generator=g)
    return B, x, uw, uh, ud, wo, wl


def dump_splines(res):
    import torch
    from flowstate import _lib

    lib, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
    for K in SPLINE_K:
        for inverse in (0, 1):
            B, x, uw, uh, ud, wo, wl = (t.cuda() if torch.is_tensor(t) else t for t in spline_case(K, inverse, 1000))
            M = x.numel()
            out, lad, gx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
            guw, guh, gud = torch.empty_like(uw), torch.empty_like(uh), torch.empty_like(ud)
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            _lib.check(lib.fs_rqs_forward_any(M, K, inverse, p(x), p(uw), p(uh), p(ud), B, p(out), p(lad), p(flag),
                                              st), "forward")
            _lib.check(lib.fs_rqs_backward_any(M, K, inverse, p(x), p(uw), p(uh), p(ud), B, p(wo), p(wl), p(gx),
                                               p(guw), p(guh), p(gud), st), "backward")
            torch.cuda.synchronize()
            for name, t in zip(("out", "lad", "gx", "guw", "guh", "gud", "nan_flag"),
                               (out, lad, gx, guw, guh, gud, flag)):
                res["rqs_K%d_inv%d_%s" % (K, inverse, name)] = t.cpu().numpy()


def dump_step(res):
    """tests/test_gpu_general_train.py::test_coupling_waves_bit_identical_at_any_k's step."""
    import torch
    from flowstate.models import build_flow, half_box
    from flowstate.normflows import autograd_flow as AF
    from flowstate.normflows.Energy import DoubleWellLJ
    from flowstate.normflows.train import step_loss

    N, kw, rows = STEP
    torch.manual_seed(2)
    B = half_box(N)
    m = build_flow(N, bound=B, device="cpu", **kw)
    m.p = DoubleWellLJ(2 * N, N, 1.0, B, V0_list=[-10.0, -10.5], r0=1.2, k=15)
    m = m.cuda().train().set_precision("f32-general")
    m.q0.device = torch.device("cuda")
    fbn = AF.FlatBatchNorm(m)
    g = np.random.default_rng(6)
    x = torch.from_numpy(((g.random((rows, 2 * N)) * 2 - 1) * B * 0.9).astype(np.float32)).cuda()
    x[::7, ::5] *= 1.2  # beyond the bound: the identity branches
    torch.cuda.manual_seed(13)
    z = m.q0(rows).cuda()
    assert AF.paired_ok(m, x, z, fbn), "the step is not on the paired coupling kernels"
    torch.cuda.manual_seed(13)
    loss = step_loss(m, x, rows, 1.0, fbn)
    loss.backward()
    torch.cuda.synchronize()
    waves = os.environ.get("FS_COUPLING_WAVES", "default")
    res["step_waves%s_loss" % waves] = loss.detach().cpu().numpy()
    for name, prm in m.named_parameters():
        if prm.grad is not None:
            res["step_waves%s_grad_%s" % (waves, name)] = prm.grad.cpu().numpy()


def dump(path, what):
    res = {}
    (dump_splines if what == "splines" else dump_step)(res)
    np.savez(path, **res)


def child(lib, path, what, waves=None):
    env = dict(os.environ, FLOWSTATE_LIB=os.path.abspath(lib))
    env.pop("FS_COUPLING_WAVES", None)
    if waves is not None:
        env["FS_COUPLING_WAVES"] = str(waves)
    subprocess.run([sys.executable, os.path.abspath(__file__), "dump", path, "--what", what], env=env, check=True,
                   timeout=300)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def compare(lib_a, lib_b, out):
    arrays = []
    with tempfile.TemporaryDirectory() as tmp:
        for lib in (lib_a, lib_b):
            got = child(lib, os.path.join(tmp, "splines.npz"), "splines")
            for waves in (0, 1):
                got.update(child(lib, os.path.join(tmp, "step%d.npz" % waves), "step", waves))
            arrays.append(got)
    a, b = arrays
    same = {k: bool(k in b and a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True)) for k in a}
    res = {"lib_a": lib_a, "lib_b": lib_b, "arrays": len(a), "same_names": sorted(a) == sorted(b),
           "spline_K": list(SPLINE_K), "spline_M": 1000, "step": {"N": STEP[0], **STEP[1], "rows": STEP[2]},
           "nan_elements": int(sum(np.isnan(v).sum() for v in a.values())),
           "different": sorted(k for k, v in same.items() if not v)}
    res["all_identical"] = res["same_names"] and not res["different"]
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
    return 0 if res["all_identical"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("compare")
    c.add_argument("lib_a")
    c.add_argument("lib_b")
    c.add_argument("--out")
    d = sub.add_parser("dump")
    d.add_argument("path")
    d.add_argument("--what", choices=("splines", "step"), required=True)
    a = ap.parse_args()
    if a.cmd == "dump":
        dump(a.path, a.what)
        return 0
    return compare(a.lib_a, a.lib_b, a.out)


if __name__ == "__main__":
    sys.exit(main())
