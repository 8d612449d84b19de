"""Chain diagnostics of the batched engine (not in the reference): how well its Markov
chains mix.  A `ChainRecorder` keeps one row per recorded step of E, W, the mean x, the
particles per well and the accept byte of every chain on the device (`fs_chain_observe`,
one launch per row); `diagnose` turns the rows into the integrated autocorrelation time
(Sokal's window) and effective sample size per chain and pooled, the Gelman-Rubin R-hat,
the mean pressure and the hops between the two wells (`fs_chain_autocov`, `fs_chain_tau`,
`fs_chain_pool`, `fs_chain_transitions`).  The definitions are in include/flowstate.h,
"Chain diagnostics".  Only the summaries leave the device."""
import math

import torch

from . import _lib

OBSERVABLES = ("E", "W", "avg_x", "wells", "accept")
FLAG_CONSTANT, FLAG_TRUNCATED, FLAG_NONFINITE = 1, 2, 4
MAX_LAG = 512
_F64 = ("E", "W", "avg_x")


class ChainRecorder:
    """[capacity][C] series of an engine's chains on its device: `E`, `W`, `avg_x` float64,
    `n_a`, `n_b` (observable "wells") and `accept` uint8; 3 * 8 + 3 * 1 bytes per chain per
    row with every observable on."""

    def __init__(self, bmc, capacity, observables=OBSERVABLES):
        unknown = set(observables) - set(OBSERVABLES)
        if unknown:
            raise ValueError(f"unknown observables {sorted(unknown)}; known: {OBSERVABLES}")
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        if bmc.N > 255:
            raise ValueError("the well counts are bytes: N <= 255")
        self.bmc, self.capacity, self.t = bmc, int(capacity), 0
        self.C, self.N = bmc.C, bmc.N
        self.half_box, self.r0 = float(bmc.phys.half_width), float(bmc.phys.r0)
        self.beta, self.volume = float(bmc.phys.beta), float(bmc.phys.box_x * bmc.phys.box_y)
        names = [k for k in _F64 if k in observables]
        names += ["n_a", "n_b"] if "wells" in observables else []
        names += ["accept"] if "accept" in observables else []
        with _lib.on_device(bmc.device):
            self._buf = {k: torch.zeros((self.capacity, self.C), dtype=torch.float64 if k in _F64 else torch.uint8,
                                        device=bmc.device) for k in names}
        self._out = _lib.ChainSeries(**{k: v.data_ptr() for k, v in self._buf.items()})

    def record(self):
        """Row `t` from the engine's live arrays (one stream-ordered launch), then t += 1."""
        if self.t >= self.capacity:
            raise RuntimeError(f"ChainRecorder is full ({self.capacity} rows); reset() or allocate more")
        b, p = self.bmc, _lib.ptr
        with _lib.on_device(b.device):
            _lib.check(_lib.load().fs_chain_observe(p(b.state), p(b.state_is_f32), p(b.E_old), p(b.W_old),
                                                    p(b.accept), self.C, self.N, self.half_box, self.r0, self.t,
                                                    self.C, self._out, _lib.stream_ptr()), "fs_chain_observe")
        self.t += 1

    def reset(self):
        self.t = 0

    def series(self):
        """The recorded rows: views [:t] of the series, plus what `diagnose` needs beside them."""
        out = {k: v[:self.t] for k, v in self._buf.items()}
        out.update(N=self.N, beta=self.beta, volume=self.volume)
        return out


def record_steps(bmc, n, recorder, local_moves=0):
    """n times: `local_moves` local moves (if any), one NF-MH step, one recorded row."""
    for _ in range(n):
        if local_moves:
            bmc.local_moves(local_moves)
        bmc.step(1)
        recorder.record()


def autocov(x, max_lag):
    """(mean [C], acov [max_lag + 1][C]) of a [T][C] float64 or uint8 device series (a
    strided view with unit column stride is taken as it is)."""
    T, C = x.shape
    if x.dtype not in (torch.float64, torch.uint8) or (C > 1 and x.stride(1) != 1):
        raise ValueError("autocov: a float64 or uint8 [T][C] series with contiguous rows")
    ld = x.stride(0) if T > 1 else max(C, 1)
    mean = torch.empty(C, dtype=torch.float64, device=x.device)
    acov = torch.empty((max_lag + 1, C), dtype=torch.float64, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.load().fs_chain_autocov(_lib.ptr(x), int(x.dtype == torch.uint8), T, C, ld, max_lag,
                                                _lib.ptr(mean), _lib.ptr(acov), _lib.stream_ptr()),
                   "fs_chain_autocov")
    return mean, acov


def tau_window(mean, acov, c=5.0):
    """(tau [C] f64, window [C] i32, flags [C] u8) of acov [W + 1][C] by Sokal's window."""
    W, C = acov.shape[0] - 1, acov.shape[1]
    tau = torch.empty(C, dtype=torch.float64, device=acov.device)
    window = torch.empty(C, dtype=torch.int32, device=acov.device)
    flags = torch.empty(C, dtype=torch.uint8, device=acov.device)
    with _lib.on_device(acov.device):
        _lib.check(_lib.load().fs_chain_tau(_lib.ptr(mean), _lib.ptr(acov), C, W, float(c), _lib.ptr(tau),
                                            _lib.ptr(window), _lib.ptr(flags), _lib.stream_ptr()), "fs_chain_tau")
    return tau, window, flags


def pool(mean, acov, T):
    """(pooled [W + 1], scalars [4]) over the chains: fs_chain_pool."""
    W, C = acov.shape[0] - 1, acov.shape[1]
    pooled = torch.zeros(W + 1, dtype=torch.float64, device=acov.device)
    scalars = torch.zeros(4, dtype=torch.float64, device=acov.device)
    with _lib.on_device(acov.device):
        _lib.check(_lib.load().fs_chain_pool(_lib.ptr(mean), _lib.ptr(acov), C, W, T, _lib.ptr(pooled),
                                             _lib.ptr(scalars), _lib.stream_ptr()), "fs_chain_pool")
    return pooled, scalars


def transitions(n_a, n_b, N):
    """[C][6] int64 {steps_A, steps_B, steps_neither, hops_AB, hops_BA, last}."""
    T, C = n_a.shape
    if n_b.shape != n_a.shape or n_b.stride() != n_a.stride() or (C > 1 and n_a.stride(1) != 1):
        raise ValueError("transitions: n_a and n_b are [T][C] uint8 series of one layout")
    out = torch.zeros((C, 6), dtype=torch.int64, device=n_a.device)
    with _lib.on_device(n_a.device):
        _lib.check(_lib.load().fs_chain_transitions(_lib.ptr(n_a), _lib.ptr(n_b), T, C,
                                                    n_a.stride(0) if T > 1 else max(C, 1), N, _lib.ptr(out),
                                                    _lib.stream_ptr()), "fs_chain_transitions")
    return out


def rhat_of(scalars, T):
    """Gelman-Rubin R-hat from fs_chain_pool's scalars (a host list); None when undefined."""
    if scalars[2] == 0.0 or scalars[3] < 2:
        return None
    return math.sqrt((T - 1) / T + scalars[1] / scalars[2])


def _observable(x, max_lag, c):
    T = x.shape[0]
    mean, acov = autocov(x, max_lag)
    tau, window, flags = tau_window(mean, acov, c)
    pooled, scalars = pool(mean, acov, T)
    tau_p, window_p, flags_p = tau_window(scalars[:1], pooled[:, None], c)
    skip = (flags == FLAG_CONSTANT) | (flags == FLAG_NONFINITE)
    ess = torch.where(skip, torch.zeros_like(tau), T / (2.0 * torch.where(skip, torch.ones_like(tau), tau)))
    counts = torch.stack([(flags == f).sum() for f in (FLAG_CONSTANT, FLAG_TRUNCATED, FLAG_NONFINITE)])
    # one copy to the host per observable: the pooled tau and the counts
    host = torch.cat([scalars, tau_p, window_p.to(torch.float64), flags_p.to(torch.float64),
                      counts.to(torch.float64)]).cpu().tolist()
    sc, tp, wp, fp = host[:4], host[4], int(host[5]), int(host[6])
    summary = dict(tau=tp, window=wp, flags=fp,
                   ess_total=(sc[3] * T / (2.0 * tp)) if fp in (0, FLAG_TRUNCATED) else 0.0,
                   rhat=rhat_of(sc, T), mean=sc[0], var_of_means=sc[1], mean_var=sc[2], n_used=int(sc[3]),
                   n_constant=int(host[7]), n_truncated=int(host[8]), n_nonfinite=int(host[9]))
    return dict(tau=tau, window=window, flags=flags, ess=ess, mean=mean, acov=acov, pooled=pooled), summary


def diagnose(recorder_or_series, max_lag=None, c=5.0):
    """Diagnostics of a recorder's rows (or of its `series()` dict).  Returns
      per_chain[name]  device tensors tau, window, flags, ess = T / (2 tau) (0 where flagged
                       constant or non-finite), mean, acov, pooled, for name in E, avg_x, accept
                       and in_a (the indicator n_a == N), whichever were recorded
      summary[name]    plain numbers: the pooled curve's tau / window / flags, ess_total =
                       n_used T / (2 tau_pooled), rhat (None when undefined), the grand mean,
                       the R-hat terms and the counts of constant / truncated / non-finite chains
      summary["pressure_mean"]  rho / beta + mean(W) / (2 V)  (monte_carlo.py:424), with W
      transitions      [C][6] int64 device table; summary["transitions"] its totals, the hop
                       rate per step over all chains and the mean residence
                       (steps_A + steps_B) / max(hops, 1)."""
    s = recorder_or_series.series() if hasattr(recorder_or_series, "series") else recorder_or_series
    first = next(v for v in s.values() if torch.is_tensor(v))
    T, C = first.shape
    if T < 1:
        raise ValueError("diagnose: no recorded rows")
    W = min(T - 1, MAX_LAG) if max_lag is None else int(max_lag)
    N = int(s["N"])
    per_chain, summary = {}, dict(T=T, C=C, N=N, max_lag=W, c=float(c))
    named = {k: s[k] for k in ("E", "avg_x", "accept") if k in s}
    if "n_a" in s:
        named["in_a"] = (s["n_a"] == N).to(torch.uint8)
    for name, x in named.items():
        per_chain[name], summary[name] = _observable(x, W, c)
    if "W" in s:
        mean_w = float(s["W"].mean())
        summary["pressure_mean"] = (N / s["volume"]) / s["beta"] + mean_w / (2.0 * s["volume"])
    res = dict(per_chain=per_chain, summary=summary)
    if "n_a" in s:
        table = transitions(s["n_a"], s["n_b"], N)
        tot = table[:, :5].sum(0).cpu().tolist()
        hops = tot[3] + tot[4]
        summary["transitions"] = dict(steps_a=tot[0], steps_b=tot[1], steps_neither=tot[2], hops_ab=tot[3],
                                      hops_ba=tot[4], hop_rate=hops / (T * C),
                                      mean_residence=(tot[0] + tot[1]) / max(hops, 1))
        res["transitions"] = table
    return res
