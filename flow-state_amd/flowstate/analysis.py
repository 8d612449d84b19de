"""Analysis reductions of the Algorithm-1 driver (hybrid_NF_MCMC/utils.py), drop-in
signatures, computed by the HIP kernels of csrc/analysis_kernels.hip:

  classify_particles(positions, halfbox, r0)                       utils.py:104-141
  calculate_well_statistics(configurations, start_idx, half_box, r0)  utils.py:61-101
  calculate_pair_correlation(final_samples, n_particles, bound, dr)   utils.py:530-574
  generate_samples(model, n_particles, n_dimension, ...)            utils.py:422-450

and the analysis batch of the Algorithm-2 driver's checkpoint cycles
(main_algorithm_2.py:485-525; fs_sample_analysis, one launch per 1000-row batch):

  sample_analysis(model, n_samples, half_box, batch=1000, bins=100, dr=None)

with, on request, the importance weights of those samples against the Boltzmann target
(ESS, log Z, reweighted heat map, g(r) and well populations; sample_analysis(reweight=...)).

Inputs are numpy arrays or device tensors; float32 and float64 inputs keep
numpy's dtype semantics (the kernels reproduce numpy 2's weak-Python-float
promotion).  The host side only does the per-configuration bookkeeping of the
reference's Python loops (running counts, p = count / i) on the device results.
"""
import numpy as np
import torch

from . import _lib

_CLASS_NAMES = np.array(["A", "B", "Outside"])


def _device_array(a):
    """(M, N, 2) float32/float64 device tensor from numpy / torch input."""
    t = torch.as_tensor(a)
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    if t.dim() == 2:
        t = t[None]
    t = t.to("cuda").contiguous()
    _lib.require_device(t)
    return t


def classify_wells(positions, halfbox, r0):
    """Device results: cls (M, N) u8 (0 A, 1 B, 2 outside), state (M,) u8
    (1 all-in-A, 2 all-in-B), avg_x (M,) f64 (np.mean of the x column)."""
    pos = _device_array(positions)
    M, N, _ = pos.shape
    cls = torch.empty((M, N), dtype=torch.uint8, device=pos.device)
    state = torch.empty(M, dtype=torch.uint8, device=pos.device)
    avg_x = torch.empty(M, dtype=torch.float64, device=pos.device)
    _lib.check(_lib.load().fs_classify_wells(_lib.ptr(pos), int(pos.dtype == torch.float32), M, N, float(halfbox),
                                             float(r0), _lib.ptr(cls), _lib.ptr(state), _lib.ptr(avg_x),
                                             _lib.stream_ptr()), "fs_classify_wells")
    return cls, state, avg_x


def classify_particles(positions, halfbox, r0):
    """utils.py:104-141: array of 'A' / 'B' / 'Outside' per particle, shape (M, N)."""
    cls, _, _ = classify_wells(positions, halfbox, r0)
    return _CLASS_NAMES[cls.cpu().numpy()]


def calculate_well_statistics(configurations, start_idx, half_box, r0=1.2):
    """utils.py:61-101: (avg_x_values, p_a_values, p_b_values, deltaF_normalized_values, runs)."""
    _, state, avg_x = classify_wells(configurations, half_box, r0)
    state = state.cpu().numpy()
    avg_x = avg_x.cpu().numpy()
    f32 = torch.as_tensor(configurations).dtype == torch.float32
    count_left = count_right = 0
    avg_x_values, p_a_values, p_b_values, deltaF, runs = [], [], [], [], []
    for i, s in enumerate(state[start_idx:], start=1):
        avg_x_values.append(np.float32(avg_x[start_idx + i - 1]) if f32 else np.float64(avg_x[start_idx + i - 1]))
        if s == 1:
            count_left += 1
        elif s == 2:
            count_right += 1
        p_a = count_left / i
        p_b = count_right / i
        p_a_values.append(p_a)
        p_b_values.append(p_b)
        deltaF.append(np.log(p_b / p_a) if (p_a > 0 and p_b > 0) else 0)
        runs.append(i)
    return avg_x_values, p_a_values, p_b_values, deltaF, runs


def pair_histograms(final_samples, bound, edges):
    """Per-configuration pair-distance counts (M, nbins) int32 on the device."""
    pos = _device_array(final_samples)
    M, N, _ = pos.shape
    e = torch.as_tensor(np.asarray(edges, np.float64), device=pos.device)
    nb = e.numel() - 1
    counts = torch.empty((M, nb), dtype=torch.int32, device=pos.device)
    _lib.check(_lib.load().fs_pair_hist(_lib.ptr(pos), int(pos.dtype == torch.float32), M, N, float(bound),
                                        _lib.ptr(e), nb, _lib.ptr(counts), _lib.stream_ptr()), "fs_pair_hist")
    return counts


def calculate_pair_correlation(final_samples, n_particles, bound, dr=None):
    """utils.py:530-574: (r_vals, g_r) with g_r a pandas Series, as the reference returns."""
    import pandas as pd

    if dr is None:
        dr = bound / 50
    edges, denom, r_vals = _rdf_bins(n_particles, bound, dr)
    counts = pair_histograms(final_samples, bound, edges)
    d = torch.as_tensor(denom, device=counts.device)
    g = torch.empty(denom.shape[0], dtype=torch.float64, device=counts.device)
    _lib.check(_lib.load().fs_rdf_mean(_lib.ptr(counts), counts.shape[0], counts.shape[1], _lib.ptr(d), _lib.ptr(g),
                                       _lib.stream_ptr()), "fs_rdf_mean")
    return r_vals, pd.Series(g.cpu().numpy())


def _rdf_bins(n_particles, bound, dr):
    """calculate_pair_correlation's edges, normalisation and r values (utils.py:559-572)."""
    edges = np.arange(0, bound + dr, dr)
    norm = n_particles * (n_particles - 1) / 2
    rou = n_particles / (4 * bound * bound)
    i_vals = np.arange(0, bound, dr)
    area = np.pi * ((i_vals + dr) ** 2 - i_vals ** 2)
    denom = norm * rou * area
    if denom.shape[0] != edges.shape[0] - 1:
        raise ValueError(f"operands could not be broadcast together with shapes ({edges.shape[0] - 1},) "
                         f"({denom.shape[0]},)")
    return edges, denom, np.arange(0, bound, dr)


def sample_analysis_batch(z, half_box, hist_edges, r_edges, samples_out, hist, counts):
    """fs_sample_analysis on one batch: z (M, N, 2) float32 device samples in centred
    coordinates; samples_out (M, N, 2) float32, hist (nb, nb) int64 (accumulated) and
    counts (M, nr) int32 are written in place (contiguous device tensors / row slices)."""
    M, N, _ = z.shape
    _lib.require_device(z, hist_edges, r_edges, samples_out, hist, counts)
    if z.dtype != torch.float32 or not z.is_contiguous():
        raise ValueError("sample_analysis_batch: z must be a contiguous float32 (M, N, 2) tensor")
    if not (samples_out.is_contiguous() and hist.is_contiguous() and counts.is_contiguous()):
        raise ValueError("sample_analysis_batch: outputs must be contiguous")
    if samples_out.shape != z.shape or counts.shape != (M, r_edges.numel() - 1) or \
            hist.numel() != (hist_edges.numel() - 1) ** 2:
        raise ValueError("sample_analysis_batch: output shapes do not match the batch")
    _lib.check(_lib.load().fs_sample_analysis(_lib.ptr(z), M, N, float(half_box), _lib.ptr(hist_edges),
                                              hist_edges.numel() - 1, _lib.ptr(r_edges), r_edges.numel() - 1,
                                              _lib.ptr(samples_out), _lib.ptr(hist), _lib.ptr(counts),
                                              _lib.stream_ptr()), "fs_sample_analysis")


def sample_analysis(model, n_samples, half_box, batch=1000, bins=100, dr=None, generator=None, reweight=None,
                    density_pass=False, r0=1.2):
    """The analysis batch of an Algorithm-2 checkpoint cycle (main_algorithm_2.py:485-525)
    on the device: ceil(n_samples / batch) batches of model.sample(batch) in eval mode
    (all n_iterations * batch rows are kept, as the reference keeps them), each through
    one fs_sample_analysis launch, then g(r) by one fs_rdf_mean; no host synchronisation
    until the results are copied out.  The base draws are made on the model's device
    (q0's uniform on [-bound, bound], `generator`: a device torch.Generator, default the
    device's own), so the host generator that orders the training batches is untouched.
    Returns a dict: samples (n, N, 2) float32 device tensor (the rows of samples.npy),
    hist (nb, nb) int64, x_edges / y_edges (np.linspace(-bound, bound, bins)), r_vals,
    g_r (numpy).

    reweight (a flowstate.MCMC.Physics whose box is 2 * half_box; default None: exactly the
    analysis above): also the importance weights w = exp(-beta E(x)) / q(x) of the same
    samples against that target and the analysis reweighted by them (include/flowstate.h
    'Importance weights').  Per batch the sampling pass hands out its log-det, and one
    energy launch, fs_classify_wells and fs_importance_weights follow fs_sample_analysis;
    after the last batch fs_weighted_reduce and fs_weighted_hist2d run over all stored rows
    with the final max_lw and S1 read on the device.  log q is the sampling pass's own
    (log q0 - sum log|det|), or with density_pass=True the density pass over
    fl32(config - half_width) exactly as BatchedMonteCarlo.proposal_terms derives it (one
    more flow pass per batch).  r0: the well radius of classify_particles.  The keys above
    are bit-identical to a call without reweight from the same generator state; added are
    log_w (f64), log_q (f32), energy (f64) (n,) device tensors; ess, ess_fraction, log_z,
    mean_log_w, max_weight_fraction (floats), n_zero, n_bad (ints); hist_w (nb, nb), g_r_w
    (numpy float64), p_a_w, p_b_w, deltaF_w, avg_x_w (floats); and the unweighted p_a, p_b,
    deltaF of the same samples (calculate_well_statistics' last values)."""
    half_box = float(half_box)
    if dr is None:
        dr = half_box / 50
    dev = next(model.parameters()).device
    N, dim = model.q0.n_particles, model.q0.n_dimension
    if dim != 2:
        raise ValueError("sample_analysis: two-dimensional particles only")
    if reweight is not None and (float(reweight.half_width) != half_box or reweight.box_y != reweight.box_x):
        raise ValueError("sample_analysis: reweight's box must be the square box of side 2 * half_box")
    n_iter = (int(n_samples) + batch - 1) // batch
    total = n_iter * batch
    x_edges = np.linspace(-half_box, half_box, bins)
    r_edges, denom, r_vals = _rdf_bins(N, half_box, dr)
    nb, nr = bins - 1, r_edges.shape[0] - 1
    was_training = model.training
    if was_training:
        model.eval()
    with _lib.on_device(dev), torch.no_grad():
        e2 = torch.as_tensor(x_edges, device=dev)
        er = torch.as_tensor(r_edges, device=dev)
        d = torch.as_tensor(denom, device=dev)
        samples = torch.empty((total, N, 2), dtype=torch.float32, device=dev)
        hist = torch.zeros((nb, nb), dtype=torch.int64, device=dev)
        counts = torch.empty((total, nr), dtype=torch.int32, device=dev)
        g = torch.empty(nr, dtype=torch.float64, device=dev)
        bound = float(model.q0.bound)
        rw = None if reweight is None else _Reweighting(model, reweight, half_box, total, density_pass, r0, dev)
        for i in range(n_iter):
            u = torch.empty((batch, N * 2), dtype=torch.float32, device=dev).uniform_(-bound, bound,
                                                                                       generator=generator)
            rows = slice(i * batch, (i + 1) * batch)
            if rw is None:
                z = model.forward(u)
            else:
                z, log_det = model.forward_and_log_det(u)  # the same launch as forward()
            z = z.reshape(batch, N, 2).contiguous()
            sample_analysis_batch(z, half_box, e2, er, samples[rows], hist, counts[rows])
            if rw is not None:
                rw.batch(samples[rows], log_det, rows)
        if total:
            _lib.check(_lib.load().fs_rdf_mean(_lib.ptr(counts), total, nr, _lib.ptr(d), _lib.ptr(g),
                                               _lib.stream_ptr()), "fs_rdf_mean")
        if rw is not None:
            rw.finish(samples, counts, d, e2, nb)
    if was_training:
        model.train()
    res = {"samples": samples, "hist": hist, "x_edges": x_edges, "y_edges": x_edges.copy(), "r_vals": r_vals,
           "g_r": g.cpu().numpy()}
    if rw is not None:
        res.update(rw.results())
    return res


def importance_summary(header):
    """ess, ess_fraction, log_z, mean_log_w, max_weight_fraction, n_zero, n_bad from the seven
    running statistics (max_lw, S1, S2, sum_lw, n, n_zero, n_bad) of an fs_importance_weights
    state block, in float64 (include/flowstate.h 'Importance weights')."""
    max_lw, s1, s2, sum_lw, n, n_zero, n_bad = header
    s1, s2, n, n_zero, n_bad = float(s1), float(s2), int(n), int(n_zero), int(n_bad)
    ess = s1 * s1 / s2 if s1 > 0 else 0.0
    finite = n - n_zero - n_bad
    return {"ess": ess, "ess_fraction": ess / n if n else 0.0,
            "log_z": float(max_lw) + float(np.log(s1 / n)) if s1 > 0 else -np.inf,
            "mean_log_w": float(sum_lw) / finite if finite else float("nan"),
            "max_weight_fraction": 1.0 / s1 if s1 > 0 else float("nan"), "n_zero": n_zero, "n_bad": n_bad}


def iw_state(device):
    """A reset fs_importance_weights state block: int64 device tensor of fs_iw_state_bytes()
    (words 0-3 hold the float64 max_lw, S1, S2, sum_lw; words 4-6 n, n_zero, n_bad)."""
    L = _lib.load()
    state = torch.empty(L.fs_iw_state_bytes() // 8, dtype=torch.int64, device=device)
    _lib.check(L.fs_iw_reset(_lib.ptr(state), _lib.stream_ptr()), "fs_iw_reset")
    return state


def iw_header(state):
    """(max_lw, S1, S2, sum_lw, n, n_zero, n_bad) of a state block, copied to the host."""
    h = state[:8].cpu()
    return tuple(h[:4].view(torch.float64).tolist()) + tuple(h[4:7].tolist())


class _Reweighting:
    """The importance-weight side of sample_analysis: per-row buffers, the state block and
    the launches, all on the caller's stream with no host synchronisation before results()."""

    def __init__(self, model, phys, half_box, total, density_pass, r0, dev):
        self.model, self.phys, self.half_box, self.r0 = model, phys, half_box, float(r0)
        self.N, self.total, self.density_pass = model.q0.n_particles, total, bool(density_pass)
        model._base_check()
        self.base = torch.tensor(model.q0.log_prob_constant(), dtype=torch.float32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        self.energy, self.log_w, self.avg_x = (torch.empty(total, **f64) for _ in range(3))
        self.log_q = torch.empty(total, dtype=torch.float32, device=dev)
        self.well = torch.empty(total, dtype=torch.uint8, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.state = iw_state(dev)

    def batch(self, cfg, log_det, rows):
        L, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
        M, N = cfg.shape[0], self.N
        E, lq, lw = self.energy[rows], self.log_q[rows], self.log_w[rows]
        _lib.check(L.fs_energy_lj_dw(self.phys.c, p(cfg), 1, M, N, p(E), None, None, None, st), "fs_energy_lj_dw")
        _lib.check(L.fs_classify_wells(p(cfg), 1, M, N, self.half_box, self.r0, None, p(self.well[rows]),
                                       p(self.avg_x[rows]), st), "fs_classify_wells")
        if self.density_pass:  # BatchedMonteCarlo.proposal_terms' log q
            x = (cfg.to(torch.float64) - self.phys.half_width).to(torch.float32).reshape(M, -1).contiguous()
            lq.copy_(self.model._log_prob(x, self.err))
        else:  # fs_flow_propose_lq's: fl32(log q0) - the sampling pass's summed log-dets, in float32
            torch.sub(self.base, log_det, out=lq)
        _lib.check(L.fs_importance_weights(float(self.phys.beta), M, p(E), p(lq), p(lw), p(self.state), st),
                   "fs_importance_weights")

    def finish(self, samples, counts, denom, edges2, nb):
        L, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
        dev, nr = samples.device, counts.shape[1]
        self.g_w = torch.zeros(nr, dtype=torch.float64, device=dev)
        self.scalars = torch.zeros(4, dtype=torch.float64, device=dev)
        self.hist_w = torch.zeros((nb, nb), dtype=torch.float64, device=dev)
        _lib.check(L.fs_weighted_reduce(p(counts), self.total, nr, p(denom), p(self.well), p(self.avg_x),
                                        p(self.log_w), p(self.state), p(self.g_w), p(self.scalars), st),
                   "fs_weighted_reduce")
        _lib.check(L.fs_weighted_hist2d(p(samples), self.total, self.N, self.half_box, p(edges2), nb, p(self.log_w),
                                        p(self.state), p(self.hist_w), st), "fs_weighted_hist2d")

    def results(self):
        if int(self.err.item()) & 4:  # (density_pass) as BatchedMonteCarlo.check_errors
            raise _lib.FlowStateError("a wide-path trunk hand-off timed out")
        res = importance_summary(iw_header(self.state))
        pa, pb, dF, ax = self.scalars.tolist()
        well = self.well.cpu().numpy()
        n = max(self.total, 1)
        p_a, p_b = int((well == 1).sum()) / n, int((well == 2).sum()) / n
        res.update(log_w=self.log_w, log_q=self.log_q, energy=self.energy, hist_w=self.hist_w.cpu().numpy(),
                   g_r_w=self.g_w.cpu().numpy(), p_a_w=pa, p_b_w=pb, deltaF_w=dF, avg_x_w=ax, p_a=p_a, p_b=p_b,
                   deltaF=float(np.log(p_b / p_a)) if (p_a > 0 and p_b > 0) else 0)
        return res


def generate_samples(model, n_particles, n_dimension, n_iterations=100, samples_per_iteration=5000,
                     device_output=False):
    """utils.py:422-450: n_iterations x model.sample(samples_per_iteration) reshaped to
    (n, n_particles, n_dimension).  device_output=True keeps the proposals on the GPU
    (one (n, N, d) float32 tensor) instead of the reference's numpy copy."""
    model.eval()
    out = []
    with torch.no_grad():
        for _ in range(n_iterations):
            z = model.sample(samples_per_iteration)
            out.append(z.reshape(-1, n_particles, n_dimension))
    if device_output:
        return torch.cat(out, 0)
    return np.concatenate([t.cpu().numpy() for t in out], axis=0)
