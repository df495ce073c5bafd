"""The reference's ars/safe_exploration.py without Ray: how tight a simulator threshold safe ARS on the swimmer needs,
as a sweep over the Lipschitz constant A and the approximation error epsilon.

The script trains a hand controller (unsafe ARS, one seed) in the real world, takes l = 0.99 x its final mean return
as the safety threshold, and then, for every A and every epsilon, n_seed safe agents that start from the hand
controller's policy, each with a simulator perturbed by epsilon and the simulator threshold l + alpha_A(H) epsilon
(ars/parameters.py Threshold.compute_alpha).  The reference starts one Ray actor per agent, 8 at a time; here

  * the hand controller goes through Experiment (one ARSAgentBatch of one seed), and
  * EVERY (A, epsilon, seed) safe agent -- 4 x 10 x 8 = 320 with the reference's sizes -- trains in ONE
    SafeARSAgentBatch: they share the real world, H, N and nu and differ in seed, simulator and simulator threshold
    only.  Agent (A, epsilon, seed) is, bit for bit, ARSAgent(safe=True, seed=seed) with that simulator.

The simulators: in the reference every actor perturbs its own copy of the real parameters with rand(3) from a freshly
started process's generator; here they are approximate_env_params(..., approx_error=epsilon) draws from `rng`, taken
in the order of the loops (A, then epsilon, then seed).

With a `guess_param` the simulators are COMPUTED instead (the reference's ARSAgent(guess_param=...) route, ars/ars_agent.py:
40-44): the hand controller's rollouts are stored, and every agent's simulator is the estimate of one estimator on that
store -- capacity 1, the agent's seed draws its rollout and seeds its search -- all of them as ONE EstimatorBatch, one
launch per CMA-ES generation for the whole sweep.

run() returns the numbers the reference plots and writes its four figures (one per A) when matplotlib imports.
Every size is an argument; the defaults are the reference's.
"""
import os

import numpy as np

from .ars_agent import approximate_env_params
from .database import Database
from .ensemble import sphere_ensemble
from .estimator_batch import EstimatorBatch
from .experiment import Experiment
from .parameters import ARSParam, EnvParam, Threshold
from .safe_agent_batch import SafeARSAgentBatch


def real_world(H=1000, epsilon=0.001):
    """The reference's real world (safe_exploration.py:22-24)."""
    return EnvParam('LeonSwimmer-RealWorld', n=3, H=H, l_i=.8, m_i=1.2, h=1e-3, k=10.2, epsilon=epsilon)


def sweep_agents(l, H, A_values, epsilons, n_seed, K, B, rng=None):
    """The agents of the sweep in batch order [A][epsilon][seed]: (seeds, sim_params, sim_thresholds, and per A the
    sim_thresh_range over the epsilons)."""
    seeds, sims, sim_thresholds, ranges = [], [], [], []
    for A in A_values:
        alpha = Threshold(K=K, A=A, B=B).compute_alpha(H)
        ranges.append(np.array([l + alpha * e for e in epsilons]))
        for epsilon in epsilons:
            sims += approximate_env_params(real_world(H, epsilon), epsilon, n_seed, rng)
            seeds += list(range(n_seed))
            sim_thresholds += [l + alpha * epsilon] * n_seed
    return seeds, sims, sim_thresholds, ranges


def hand_controller(*, hand_iter, H, N, b, alpha, nu, results_path, data_path, store=False):
    """The first stage of the script, shared by run() and run_ensemble(): the hand controller (unsafe ARS V1, one
    seed, from zero weights) trained in the real world, its policy saved, and the safety threshold l = 0.99 x its
    final mean return written to data_path + threshold.txt.  store: keep its rollouts (hand_trajectories.npz).
    -> (the real world's EnvParam, l, results_path and the policy's path without '.npy', the store's path or None)."""
    results_path, data_path = os.path.join(results_path, ""), os.path.join(data_path, "")   # Experiment appends to it
    os.makedirs(results_path, exist_ok=True)
    os.makedirs(data_path, exist_ok=True)
    ep = real_world(H)

    # the initial weights, as if from a hand controller (safe_exploration.py:28-36)
    hand_agent = ARSParam('HandControl', V1=True, n_iter=hand_iter, H=H, N=N, b=b, alpha=alpha, nu=nu, safe=False,
                          threshold=0, initial_w='Zero')
    policy_path = os.path.join(data_path, "saved_hand_policy")
    store_path = os.path.join(data_path, "hand_trajectories.npz") if store else None
    returns = Experiment(ep, results_path=results_path, save_data_path=store_path,
                         save_policy_path=policy_path).plot(n_seed=1, agent_param=hand_agent)
    # the safety threshold from the known controller (:39-42)
    l = float(np.mean(returns, axis=0)[-1] * 0.99)
    print(f"\nSafety threshold: {l}")
    np.savetxt(os.path.join(data_path, "threshold.txt"), np.array([l]))
    return ep, l, results_path, policy_path, store_path


def summarise(r_graphs):
    """(min_return, max_mean_returns) over the epsilons of r_graphs [eps][seed][n_iter + 1] (safe_exploration.py:80-82)."""
    return (np.array([np.nanmin(r) for r in r_graphs]),
            np.array([np.nanmax(np.mean(r, axis=0)) for r in r_graphs]))


def run(*, A_values=(0.1, 0.3, 0.5, 0.7), epsilons=None, n_seed=8, n_iter=400, hand_iter=200, H=1000, K=1, B=0.001,
        N=1, b=1, alpha=0.0075, nu=0.01, results_path="results/", data_path="ars/data/", rng=None, device=None,
        guess_param=None, estimator_options=None):
    """The whole script.  Returns a dict: l, epsilons, A_values, and per A (lists in the order of A_values)
    min_return [n_eps], max_mean_returns [n_eps], sim_thresh_range [n_eps]; r_graphs [A][eps][seed][n_iter + 1];
    sim_params, the agents' simulators in batch order.
    Files: data_path + saved_hand_policy.npy and threshold.txt, the hand controller's Experiment files under
    results_path, and results_path + epsilon_sim_threshold_H=.._K=.._A=.._B=...png per A.
    guess_param (an EnvParam with the real world's n, h and H): estimate every agent's simulator from the hand
    controller's stored rollouts (data_path + hand_trajectories.npz) with one EstimatorBatch, starting at the guess;
    estimator_options are passed to EstimatorBatch.estimate."""
    epsilons = np.linspace(0.0001, 0.01, 10) if epsilons is None else np.asarray(epsilons, dtype=np.float64)
    A_values = list(A_values)
    ep, l, results_path, policy_path, store_path = hand_controller(
        hand_iter=hand_iter, H=H, N=N, b=b, alpha=alpha, nu=nu, results_path=results_path, data_path=data_path,
        store=guess_param is not None)

    # every safe agent of the sweep in one batch (:54-82)
    seeds, sims, sim_thresholds, ranges = sweep_agents(l, H, A_values, epsilons, n_seed, K, B, rng)
    if guess_param is not None:   # computed simulators: one estimator per agent, all searches in lock-step
        store = Database()
        store.load(store_path)
        sims = EstimatorBatch(store, guess_param, capacity=1, seeds=seeds,
                              device=device or "cuda:0").estimate(**(estimator_options or {}))
    real_agent = ARSParam('RLControl', V1=True, n_iter=n_iter, H=H, N=N, b=b, alpha=alpha, nu=nu, safe=True,
                          threshold=l, initial_w=policy_path + ".npy")
    batch = SafeARSAgentBatch(ep, real_agent, seeds, sims, sim_thresholds, device=device)
    curves = batch.runTraining()
    r_graphs = curves.reshape(len(A_values), len(epsilons), n_seed, n_iter + 1)
    out = dict(l=l, epsilons=epsilons, A_values=A_values, r_graphs=r_graphs, sim_thresh_range=ranges, sim_params=sims,
               min_return=[], max_mean_returns=[], violations=batch.violations.reshape(r_graphs.shape[:3]))
    for g in r_graphs:
        lo, hi = summarise(g)
        out["min_return"].append(lo)
        out["max_mean_returns"].append(hi)
    _figures(out, H, K, B, results_path)
    return out


def run_ensemble(*, epsilons=None, n_seed=8, n_sim=8, n_iter=400, hand_iter=200, H=1000, N=1, b=1, alpha=0.0075,
                 nu=0.01, results_path, data_path, rng=None, ensemble_rng=None, device=None):
    """The sweep without Lipschitz constants: the hand-controller stage of run(), then all len(epsilons) * n_seed safe
    agents as ONE SafeARSAgentBatch whose gate runs in an ensemble of n_sim simulators per agent.  Agent (epsilon,
    seed) draws its centre as run() draws its simulator (approximate_env_params from `rng`, in the order epsilon, then
    seed), its ensemble is sphere_ensemble(centre, epsilon, n_sim, ensemble_rng), and its simulator threshold is l
    itself: the worst member stands where alpha_A(H) * epsilon stood.
    Returns run()'s dictionary without the A axis -- l, epsilons, r_graphs [eps][seed][n_iter + 1], min_return,
    max_mean_returns, sim_thresh_range (l for every epsilon) [n_eps], violations [eps][seed], sim_params (the centres)
    -- plus sim_ensembles [eps * seed][n_sim] and worst_margin [n_eps]: the minimum over seeds and iterations of
    worst - l over the admitted directions (+inf where nothing was admitted).  One figure, when matplotlib imports."""
    epsilons = np.linspace(0.0001, 0.01, 10) if epsilons is None else np.asarray(epsilons, dtype=np.float64)
    ep, l, results_path, policy_path, _ = hand_controller(hand_iter=hand_iter, H=H, N=N, b=b, alpha=alpha, nu=nu,
                                                          results_path=results_path, data_path=data_path)
    seeds, centres, ensembles = [], [], []
    for epsilon in epsilons:
        drawn = approximate_env_params(real_world(H, epsilon), epsilon, n_seed, rng)
        centres += drawn
        ensembles += [sphere_ensemble(c, epsilon, n_sim, ensemble_rng) for c in drawn]
        seeds += list(range(n_seed))
    real_agent = ARSParam('RLControl', V1=True, n_iter=n_iter, H=H, N=N, b=b, alpha=alpha, nu=nu, safe=True,
                          threshold=l, initial_w=policy_path + ".npy")
    batch = SafeARSAgentBatch(ep, real_agent, seeds, None, [l] * len(seeds), device=device, sim_ensembles=ensembles)
    r_graphs = batch.runTraining().reshape(len(epsilons), n_seed, n_iter + 1)
    lo, hi = summarise(r_graphs)
    out = dict(l=l, epsilons=epsilons, r_graphs=r_graphs, sim_thresh_range=np.full(len(epsilons), l),
               sim_params=centres, sim_ensembles=ensembles, min_return=lo, max_mean_returns=hi,
               violations=batch.violations.reshape(r_graphs.shape[:2]),
               worst_margin=(batch.min_admitted_worst - l).reshape(r_graphs.shape[:2]).min(axis=1))
    _figures(dict(out, A_values=["ensemble"], min_return=[lo], max_mean_returns=[hi], sim_thresh_range=[out["sim_thresh_range"]]),
             H, None, None, results_path, name=f"epsilon_ensemble_H={H}_E={n_sim}.png",
             title=f"Safe ARS gated by an ensemble of {n_sim} simulators on the epsilon-sphere, H={H}")
    return out


def _figures(out, H, K, B, results_path, name=None, title=None):
    """The reference's figure per A (safe_exploration.py:85-100) on Agg canvases of their own, as Experiment._figures
    draws its own; skipped when matplotlib does not import."""
    try:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
    except ImportError:
        return
    eps, l = out["epsilons"], out["l"]
    for i, A in enumerate(out["A_values"]):
        fig = Figure(figsize=(10, 8))
        FigureCanvasAgg(fig)
        axes = fig.add_subplot(111)
        axes.plot(eps, out["min_return"][i], marker='o', label="Minimum return")
        axes.plot(eps, out["max_mean_returns"][i], marker='o', label="Max of mean learning curve")
        axes.plot(eps, out["sim_thresh_range"][i], linestyle='--', marker='D', label="Simulator threshold")
        axes.plot(eps, [l] * len(eps), color='black', linewidth=2, label="Safety threshold")
        axes.legend()
        axes.set_xlabel("epsilon")
        axes.set_ylabel("Average return")
        axes.set_title(title or
                       f"Safe ARS with approximation error of epsilon, with constants H={H}, K={K}, A={A}, B={B}")
        fig.savefig(os.path.join(results_path, name or f"epsilon_sim_threshold_H={H}_K={K}_A={A}_B={B}.png"))
