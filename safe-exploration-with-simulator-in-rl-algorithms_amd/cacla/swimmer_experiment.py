"""CACLA on the swimmer over a grid of hyper-parameters: the reference's cacla/swimmer_experiment.py:21-57 without
Ray.  Where the reference starts one Ray task per (gamma, alpha, sigma) and trains that task's seeds one after the
other, the whole grid -- every setting times every seed -- is ONE CACLABatch: one launch per chunk of steps.

Seeds: the reference seeds nothing (each Ray worker starts from its own entropy); here the agents of a setting are
seeded 0 .. n_seed - 1, so a curve can be reproduced, and grid() gives for a setting what experience() gives.

Files, under out_dir (created when missing; the reference's "results/cacla/"): `<stem>.npy` with the setting's
rewards [n_seed, n_iter] and -- when matplotlib imports -- `<stem>.png`, the reference's figure (:36-44), with
<stem> = gamma=<round(gamma, 3)>_alpha=<alpha>_sigma=<sigma> as there.
"""
import os

import numpy as np

from .cacla_agent import CACLABatch


def stem(gamma, alpha, sigma):
    return f"gamma={round(float(gamma), 3)}_alpha={alpha}_sigma={sigma}"


def _curve(rewards):
    """mean and std over the seeds as the reference takes them (:31-32): a diverged seed's NaN is left out."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)    # a step at which every seed is NaN
        return np.nanmean(rewards, axis=0), np.nanstd(rewards, axis=0)


def _figure(env, gamma, alpha, sigma, H, mean, std, path):
    try:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
    except ImportError:
        return
    n_iter = len(mean)
    t = np.linspace(0, n_iter, n_iter)
    fig = Figure()
    FigureCanvasAgg(fig)
    axes = fig.add_subplot(111)
    axes.plot(t, mean, color="#CC4F1B", label=f"gamma={round(float(gamma), 3)}, alpha={alpha}, sigma={sigma}")
    axes.fill_between(t, mean - std, mean + std, alpha=0.5, edgecolor="#CC4F1B", facecolor="#FF9848")
    axes.legend()
    axes.set_xlabel("Timesteps")
    axes.set_ylabel(f"Sum of last {H} rewards")
    axes.set_title(f"CACLA on {env.envName} learning curve")
    fig.savefig(path)


def grid(env, gammas, alphas, sigmas, n_iter, n_seed=3, out_dir="results/cacla/", H=1000, chunk=2048):
    """Every (gamma, alpha, sigma) of the three lists (gamma slowest, as the reference's loop, :55) with n_seed
    agents each, trained together.  Returns {(gamma, alpha, sigma): (mean [n_iter], std [n_iter])}; out_dir None
    writes no files."""
    settings = [(g, a, s) for g in gammas for a in alphas for s in sigmas]
    if not settings or n_seed < 1:
        raise ValueError("grid needs at least one setting and one seed")
    per_agent = [st for st in settings for _ in range(n_seed)]
    batch = CACLABatch(env, [st[0] for st in per_agent], [st[1] for st in per_agent], [st[2] for st in per_agent],
                       list(range(n_seed)) * len(settings))
    rewards = batch.run(n_iter, chunk=chunk).reshape(len(settings), n_seed, n_iter)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    curves = {}
    for (g, a, s), r in zip(settings, rewards):
        mean, std = _curve(r)
        curves[(g, a, s)] = (mean, std)
        print(f"Last mean reward obtained for gamma={round(float(g), 3)}, alpha={a}, sigma={s}: "
              f"{mean[-1] if n_iter else float('nan')}")
        if out_dir is not None:
            np.save(os.path.join(out_dir, stem(g, a, s)), r)
            _figure(env, g, a, s, H, mean, std, os.path.join(out_dir, stem(g, a, s) + ".png"))
    return curves


def safe_compare(env, sim, gamma, alpha, sigma, seeds, cost, real_threshold, sim_threshold, n_iter, chunk=2048):
    """Plain against safe exploration from the same seeds: per seed one ungated agent and one agent gated by the
    simulator `sim` (a SwimmerEnv with env's n, h and direction), all in ONE CACLA_SE_Batch.  Both agents of a seed
    start from the same weights and see the same noise, so they part only where the gate refuses a step.

    Returns a dict: rewards_plain, rewards_safe [n_seed, n_iter] (safe: NaN before a seed's first admitted step, a
    refused step repeats the last reward), violations_plain, violations_safe, admitted_plain, admitted_safe [n_seed]
    and first_refused [n_seed] (the safe agents'; -1: nothing refused)."""
    from .cacla_safe_swimmer import CACLA_SE_Batch, _same_model
    _same_model(env, sim)
    seeds = [int(s) for s in seeds]
    S = len(seeds)
    if S < 1:
        raise ValueError("safe_compare needs at least one seed")
    batch = CACLA_SE_Batch(env, [gamma] * 2 * S, [alpha] * 2 * S, [sigma] * 2 * S, seeds + seeds,
                           [[sim.l_i, sim.m_i, sim.k]] * 2 * S, [sim_threshold] * 2 * S, [real_threshold] * 2 * S,
                           cost, gated=[0] * S + [1] * S)
    rewards, _ = batch.run(n_iter, chunk=chunk)
    return dict(rewards_plain=rewards[:S], rewards_safe=rewards[S:],
                violations_plain=batch.violations[:S].copy(), violations_safe=batch.violations[S:].copy(),
                admitted_plain=batch.admitted[:S].copy(), admitted_safe=batch.admitted[S:].copy(),
                first_refused=batch.first_refused[S:].copy())


def safe_compare_ensemble(env, ensemble, gamma, alpha, sigma, seeds, cost, real_threshold, n_iter, sim_threshold=None,
                          chunk=2048):
    """Plain, gated on one simulator and gated on an ensemble of simulators from the same seeds: per seed one ungated
    agent, one gated on member 0 of `ensemble` alone (as E copies of it: the ensemble kernel then has the single
    kernel's bits) and one gated on all E members -- all three in ONE CACLA_SE_Batch.  `ensemble` is what
    CACLA_SE_agent's sim_ensemble takes; sim_threshold None is the real threshold itself.

    Returns a dict: rewards_*, admitted_*, violations_* and first_refused_* (-1: nothing refused) for plain / single /
    ensemble ([n_seed, n_iter] the rewards, [n_seed] the rest), member_refusals [n_seed, E] (the ensemble agents':
    which member binds) and worst_margin [n_seed]: the smallest sim_threshold - worst_cost over the ensemble agent's
    admitted steps, +inf where none was admitted -- how close the worst member came to the threshold."""
    from .cacla_safe_swimmer import CACLA_SE_Batch, _ensemble, member_rows
    rows = member_rows(env, _ensemble(ensemble))
    seeds = [int(s) for s in seeds]
    S, E = len(seeds), len(rows)
    if S < 1:
        raise ValueError("safe_compare_ensemble needs at least one seed")
    if sim_threshold is None:
        sim_threshold = real_threshold
    members = np.concatenate([np.tile(rows[:1], (2 * S, E, 1)), np.tile(rows, (S, 1, 1))])
    batch = CACLA_SE_Batch(env, [gamma] * 3 * S, [alpha] * 3 * S, [sigma] * 3 * S, seeds * 3, None,
                           [sim_threshold] * 3 * S, [real_threshold] * 3 * S, cost, gated=[0] * S + [1] * 2 * S,
                           sim_ensembles=members)
    rewards, admitted = batch.run(n_iter, chunk=chunk)
    out = {}
    for i, who in enumerate(("plain", "single", "ensemble")):
        part = slice(i * S, (i + 1) * S)
        out["rewards_" + who] = rewards[part]
        out["admitted_" + who] = batch.admitted[part].copy()
        out["violations_" + who] = batch.violations[part].copy()
        out["first_refused_" + who] = batch.first_refused[part].copy()
    out["member_refusals"] = batch.member_refusals[2 * S:].copy()
    margin = np.where(admitted[2 * S:], float(sim_threshold) - batch.worst_cost[2 * S:], np.inf)
    out["worst_margin"] = margin.min(axis=1, initial=np.inf)
    return out


def experience(env, gamma, alpha, sigma, n_iter, H=1000, n_seed=3, out_dir="results/cacla/"):
    """One setting of the grid (swimmer_experiment.py:21-44): (t, mean, std) of its n_seed agents."""
    mean, std = grid(env, [gamma], [alpha], [sigma], n_iter, n_seed=n_seed, out_dir=out_dir, H=H)[(gamma, alpha, sigma)]
    return np.linspace(0, n_iter, n_iter), mean, std
