"""Output formats of the Algorithm-1 driver (hybrid_NF_MCMC/main_algorithm_1.py),
written from the batched engine's device results:

  sample tuples            MonteCarlo.sample (MCMC/monte_carlo.py:416-444)
  sampled_data.csv         main_algorithm_1.py:499-534 (one row per sample() tuple)
  mc_run_configs.npy       main_algorithm_1.py:537-541 (stacked sample configurations)
  mc_run_testing_configs.npy  main_algorithm_1.py:544-547
  params.json              main_algorithm_1.py:131-134 (json, indent 4)
  acceptance_rate_data.csv main_algorithm_1.py:434-440
  model .pth               torch.save(model.state_dict()) (main_algorithm_1.py:327)

and of the Algorithm-2 driver's checkpoint cycles (hybrid_NF_MCMC/main_algorithm_2.py):

  samples.npy                                    main_algorithm_2.py:504-505
  frequency_heatmap_cycle_{c}_data.json          utils.py:495-506
  pair_correlation_function_{c}_data.json        utils.py:599-606
  loss_function_data.json                        utils.py:403-406
  model_checkpoint_cycle_{c}.pth                 main_algorithm_2.py:468-470
  p_acc_history_data.json                        main_algorithm_2.py:588-599
  importance_cycle_{c}_data.json                 (not the reference's: Algorithm2(reweight_analysis=True))
  chain_diagnostics_data.json                    (not the reference's: diagnostics.diagnose)

The batched engine returns sample() snapshots as device arrays (E, W and the
configuration at each sampled step); `sample_tuples` turns one chain's snapshots
into the reference's tuples with the reference's arithmetic.
"""
import csv
import json
import os

import numpy as np


def sample_tuple(cycle_number, total_energy, total_virial, num_particles, box_x, box_y, beta, particles):
    """(cycle, E/N, rho, P, box_x, box_y, particles) as monte_carlo.py:420-444 computes it."""
    volume = box_x * box_y  # SimulationBox.volume (simulation_box.py:17)
    energy_per_particle = total_energy / num_particles
    density = num_particles / volume
    pressure = density / beta + total_virial / (2.0 * volume)
    return (cycle_number, energy_per_particle, density, pressure, box_x, box_y, np.array(particles, copy=True))


def sample_tuples(bmc, samples_xy, samples_ew, chain, step0, sample_every, n_moves):
    """One chain's sample() tuples from BatchedMonteCarlo.local_moves(..., sample_every)
    outputs; particles come back in the chain's reference dtype."""
    steps = [s for s in range(step0 + 1, step0 + n_moves + 1) if s % sample_every == 0]
    xy = samples_xy[chain].cpu().numpy()
    ew = samples_ew[chain].cpu().numpy()
    f32 = bool(bmc.state_is_f32[chain].item())
    out = []
    for k, s in enumerate(steps):
        p = xy[k].astype(np.float32) if f32 else xy[k]
        out.append(sample_tuple(s, np.float64(ew[k, 0]), np.float64(ew[k, 1]), bmc.N, np.float64(bmc.phys.box_x),
                                np.float64(bmc.phys.box_y), bmc.phys.beta, p))
    return out


def write_sampled_data(path, local_samples):
    """sampled_data.csv of one run (main_algorithm_1.py:499-534)."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["cycle_number", "energy_per_particle", "density", "pressure", "box_size_x", "box_size_y",
                    "particle_configuration"])
        for cycle, epp, rho, p, bx, by, particles in local_samples:
            w.writerow([cycle, epp, rho, p, bx, by, np.array(particles).flatten().tolist()])


def save_configs(path, samples):
    """mc_run_configs.npy / mc_run_testing_configs.npy: np.array of the configurations
    (sample[6] of each tuple, or the configurations themselves)."""
    cfgs = [s[6] if isinstance(s, tuple) else s for s in samples]
    np.save(path, np.array(cfgs))


def write_params(path, params):
    with open(path, "w") as f:
        json.dump(params, f, indent=4)


def write_acceptance_rate(path, steps_history, p_acc_history):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["MCMC_Steps", "Acceptance_Rate"])
        for s, a in zip(steps_history, p_acc_history):
            w.writerow([s, a])


# ---------------------------------------------------------------- Algorithm 2
# The data files of main_algorithm_2.py's checkpoint cycles (the reference writes each
# next to a plot; the plots stay out of scope).

def _tolist(a):
    return a.tolist() if hasattr(a, "tolist") else list(a)


def save_samples(directory, samples):
    """samples.npy (main_algorithm_2.py:504-505): the analysis batch, float32 (n, N, 2)."""
    a = samples.cpu().numpy() if hasattr(samples, "cpu") else np.asarray(samples)
    path = os.path.join(directory, "samples.npy")
    np.save(path, a)
    return path


def write_frequency_heatmap(directory, cycle, hist, x_edges, y_edges, cmap_name=None):
    """frequency_heatmap_cycle_{cycle}_data.json (utils.py:495-506): the histogram2d
    counts normalised in float64."""
    hist = (hist.cpu().numpy() if hasattr(hist, "cpu") else np.asarray(hist)).astype(np.float64)
    data = {"hist_relative": (hist / hist.sum()).tolist(), "x_edges": _tolist(x_edges), "y_edges": _tolist(y_edges),
            "cmap_name": cmap_name}
    path = os.path.join(directory, f"frequency_heatmap_cycle_{cycle}_data.json")
    with open(path, "w") as f:
        json.dump(data, f)
    return path


def write_pair_correlation(directory, cycle, r_vals, g_r):
    """pair_correlation_function_{cycle}_data.json (utils.py:599-606); `directory` is stored
    with the trailing separator the reference passes."""
    g = g_r.values if hasattr(g_r, "values") else g_r
    data = {"r": _tolist(r_vals), "g_r": _tolist(g), "directory": str(directory) + "/"}
    path = os.path.join(directory, f"pair_correlation_function_{cycle}_data.json")
    with open(path, "w") as f:
        json.dump(data, f)
    return path


IMPORTANCE_SCALARS = ("ess", "ess_fraction", "log_z", "mean_log_w", "max_weight_fraction", "n_zero", "n_bad", "p_a_w",
                      "p_b_w", "deltaF_w", "avg_x_w", "p_a", "p_b", "deltaF")


def write_importance(directory, cycle, res):
    """importance_cycle_{cycle}_data.json: the importance-weight scalars of an analysis batch
    (analysis.sample_analysis(reweight=...)), the reweighted g(r) over r and the reweighted
    heat map (sum of the normalised weights per bin) with its edges."""
    data = {k: res[k] for k in IMPORTANCE_SCALARS}
    data.update(r=_tolist(res["r_vals"]), g_r_w=_tolist(res["g_r_w"]), hist_w=_tolist(res["hist_w"]),
                x_edges=_tolist(res["x_edges"]), y_edges=_tolist(res["y_edges"]))
    path = os.path.join(directory, f"importance_cycle_{cycle}_data.json")
    with open(path, "w") as f:
        json.dump(data, f)
    return path


def write_chain_diagnostics(directory, result):
    """chain_diagnostics_data.json: the summary of diagnostics.diagnose (plain floats, ints and
    None: per observable the pooled tau and window, ess_total, rhat, the grand mean and the
    counts of flagged chains; the mean pressure; the well-hop totals)."""
    path = os.path.join(directory, "chain_diagnostics_data.json")
    with open(path, "w") as f:
        json.dump(result["summary"], f)
    return path


def write_tempering(directory, summary):
    """tempering_data.json: TemperedMonteCarlo.swap_summary() (plain floats, ints and lists:
    per rung pair the exchange attempts, accepts and rate; the round trips per ladder and in
    total; per temperature the mean energy, the move acceptance and the well populations)."""
    path = os.path.join(directory, "tempering_data.json")
    with open(path, "w") as f:
        json.dump(summary, f)
    return path


def save_model_checkpoint(directory, cycle, model):
    """model_checkpoint_cycle_{cycle}.pth (main_algorithm_2.py:469-470)."""
    import torch

    path = os.path.join(directory, f"model_checkpoint_cycle_{cycle}.pth")
    torch.save(model.state_dict(), path)
    return path


def write_loss_history(directory, loss_epoch, base_filename="loss_function"):
    """loss_function_data.json (utils.py:403-406)."""
    path = os.path.join(directory, f"{base_filename}_data.json")
    with open(path, "w") as f:
        json.dump({"loss_epoch": _tolist(loss_epoch)}, f)
    return path


def write_p_acc_history(directory, p_acc_history, initial_training_num_samples, update_num_samples):
    """p_acc_history_data.json (main_algorithm_2.py:588-599): p_acc_history is the initial
    acceptance followed by one entry per cycle; total_samples_trained has as many entries."""
    total = [initial_training_num_samples]
    for _ in range(1, len(p_acc_history)):
        total.append(total[-1] + update_num_samples)
    path = os.path.join(directory, "p_acc_history_data.json")
    with open(path, "w") as f:
        json.dump({"total_samples_trained": total, "p_acc_history": list(p_acc_history)}, f, indent=4)
    return path


def write_run_dir(run_dir, local_samples, testing_samples=None):
    """The per-run files of main_algorithm_1.py:499-547."""
    os.makedirs(run_dir, exist_ok=True)
    write_sampled_data(os.path.join(run_dir, "sampled_data.csv"), local_samples)
    save_configs(os.path.join(run_dir, "mc_run_configs.npy"), local_samples)
    save_configs(os.path.join(run_dir, "mc_run_testing_configs.npy"), testing_samples or [])
