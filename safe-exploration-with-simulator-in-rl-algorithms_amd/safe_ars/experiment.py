"""safe_ars/experiment.py of the reference without its module-level side effects: a real swimmer (m, l, k) =
(1, 1, 10), a simulator at distance epsilon, the cost "maximum speed angle", and per seed a Basic_ARS and a Safe_ARS
agent trained from the same seed -- here all 2 n_seeds agents as ONE `ARSBatch`.

    python -m swimmer_amd.safe_ars.experiment --epsilon 0.05 --thresh 3 --n_iter 100 --n_rollout 1000 --N 8 --b 4 \\
        --alpha 0.02 --nu 0.03 --path ./ --n_seeds 10

`run` returns what the script accumulates and plots; `main` takes the script's ten flags and saves its figure.
`run_ensemble` adds a third agent per seed, gated on an ensemble of simulators on the epsilon-sphere around the estimate
(where the script has one simulator and `sim_thresh = thresh - 1`, :59), all 3 n_seeds agents in one batch.
"""
import argparse

import numpy as np

from ..envs import SwimmerEnv
from .ars import MaxAbsThetaDot
from .batch import ARSBatch

N_SEGMENTS = 3
THETA_REAL = (1.0, 1.0, 10.0)          # (m_i, l_i, k), experiment.py:31-33


def draw_setup(epsilon, n_iter, N, n_seeds, seeds=None, theta_sim=None):
    """(theta_sim, seeds) as the script would draw them from NumPy's global generator in its current state -- rand(3)
    for the simulator's direction (:36-37), then seed 0 = randint(2**32 - 1) and seed i + 1 = the same draw from seed
    i's stream behind the n_iter * N * m * d doubles of the safe agent's training (:59-66, :77) -- on RandomState
    objects, and the global generator left where the script would leave it.  Given values are used as they are and
    draw nothing."""
    m, d = N_SEGMENTS - 1, 2 * N_SEGMENTS + 2
    if theta_sim is None or seeds is None:
        rs = np.random.RandomState()
        rs.set_state(np.random.get_state())
        if theta_sim is None:
            delta = rs.rand(len(THETA_REAL))
            theta_sim = np.array(THETA_REAL) + delta / np.linalg.norm(delta, ord=2) * epsilon
        if seeds is None:
            seeds = []
            for _ in range(n_seeds):
                seeds.append(int(rs.randint(2 ** 32 - 1)))
                rs = np.random.RandomState(seeds[-1])
                rs.random_sample(n_iter * N * m * d)       # both agents of a seed draw the same deltas
        np.random.set_state(rs.get_state())
    seeds = [int(s) for s in seeds]
    if len(seeds) != n_seeds:
        raise ValueError(f"seeds: expected {n_seeds}, got {len(seeds)}")
    return np.asarray(theta_sim, dtype=np.float64), seeds


def run(epsilon, thresh, n_iter, n_rollout, N, b, alpha, nu, n_seeds, seeds=None, theta_sim=None, device=None,
        rollout_kernel="auto"):
    """The whole experiment.  Returns a dict: theta_sim, seeds, the per-seed arrays unsafe_returns / safe_returns
    [n_seeds, n_iter] and unsafe_costs / safe_costs [n_seeds, 2 n_iter n_rollout] (the script's `all_*` lists), the
    script's mean_* and std_* arrays, per-seed real-threshold violation counts (the script prints each violation) and
    the trained ARSBatch (`batch`: agent 2i is seed i's basic agent, 2i + 1 its safe one)."""
    theta_sim, seeds = draw_setup(epsilon, n_iter, N, n_seeds, seeds, theta_sim)
    kw = {} if device is None else {"device": device}
    real_env = SwimmerEnv("RealWorld", n=N_SEGMENTS, m_i=THETA_REAL[0], l_i=THETA_REAL[1], k=THETA_REAL[2], **kw)
    sim_env = SwimmerEnv("Simulator", n=N_SEGMENTS, m_i=theta_sim[0], l_i=theta_sim[1], k=theta_sim[2], **kw)
    batch = ARSBatch(real_env, [s for s in seeds for _ in range(2)], [False, True] * n_seeds, MaxAbsThetaDot(),
                     real_thresh=thresh, sim_thresh=thresh - 1, sim_envs=sim_env, device=device,
                     rollout_kernel=rollout_kernel)
    curves = batch.train(n_iter, N, b, alpha, nu, n_rollout, costs="reference")
    out = {"theta_sim": theta_sim, "seeds": seeds, "batch": batch,
           "unsafe_returns": curves[0::2], "safe_returns": curves[1::2],
           "unsafe_costs": batch.costs[0::2], "safe_costs": batch.costs[1::2],
           "unsafe_violations": batch.real_violations[0::2], "safe_violations": batch.real_violations[1::2]}
    for kind in ("unsafe", "safe"):
        out[f"mean_{kind}_returns"] = np.mean(out[f"{kind}_returns"], axis=0)
        out[f"mean_{kind}_costs"] = np.mean(out[f"{kind}_costs"], axis=0)
        out[f"std_{kind}_returns"] = np.std(out[f"{kind}_returns"], axis=0)
    return out


def ensemble_members(theta_sim, epsilon, n_sim, ensemble_seed=0):
    """[n_sim, 3] (m_i, l_i, k): member 0 is theta_sim, member i >= 1 theta_sim + epsilon g / ||g||_2 with
    g = RandomState(ensemble_seed).standard_normal(3) drawn in member order -- samples on the epsilon-sphere around the
    estimate, the sphere that holds the real swimmer by construction.  No global generator is touched."""
    n_sim = int(n_sim)
    if n_sim < 1:
        raise ValueError("ensemble_members needs n_sim >= 1")
    rs = np.random.RandomState(ensemble_seed)
    rows = [np.asarray(theta_sim, dtype=np.float64)]
    for _ in range(1, n_sim):
        g = rs.standard_normal(3)
        rows.append(rows[0] + epsilon * (g / np.linalg.norm(g, ord=2)))
    return np.array(rows)


def run_ensemble(epsilon, thresh, n_iter, n_rollout, N, b, alpha, nu, n_seeds, n_sim, seeds=None, theta_sim=None,
                 ensemble_seed=0, sim_thresh=None, device=None):
    """The experiment with a third agent per seed, gated on an ENSEMBLE of n_sim simulators (ensemble_members) at
    sim_thresh (default: `thresh` itself) where the script's safe agent is gated on one simulator at `thresh - 1`.  Per
    seed a basic agent, the script's safe agent (n_sim copies of member 0) and the ensemble agent train in ONE ARSBatch
    (agents 3i, 3i + 1, 3i + 2), so setup and seeds are drawn as `run` draws them.  Returns run's keys for the first two
    -- the bits of run(..., rollout_kernel="lane") on the same seeds and theta_sim -- and for the ensemble agent
    ensemble_returns [n_seeds, n_iter], ensemble_costs [n_seeds, 2 n_iter n_rollout], ensemble_violations [n_seeds],
    member_refusals [n_seeds, n_sim] (the rollouts in which member e was among those that refused), worst_margin (the
    simulator threshold minus the largest member cost of any admitted step of the ensemble agents: how far the worst
    member stayed from the threshold; the threshold itself where nothing was admitted) and `members` [n_sim, 3]."""
    theta_sim, seeds = draw_setup(epsilon, n_iter, N, n_seeds, seeds, theta_sim)
    sim_thresh = thresh if sim_thresh is None else sim_thresh
    kw = {} if device is None else {"device": device}
    real_env = SwimmerEnv("RealWorld", n=N_SEGMENTS, m_i=THETA_REAL[0], l_i=THETA_REAL[1], k=THETA_REAL[2], **kw)
    members = ensemble_members(theta_sim, epsilon, n_sim, ensemble_seed)
    sims = [SwimmerEnv("Simulator", n=N_SEGMENTS, m_i=row[0], l_i=row[1], k=row[2], **kw) for row in members]
    batch = ARSBatch(real_env, [s for s in seeds for _ in range(3)], [False, True, True] * n_seeds, MaxAbsThetaDot(),
                     real_thresh=thresh, sim_thresh=[0.0, thresh - 1, sim_thresh] * n_seeds, device=device,
                     sim_ensembles=[None, [sims[0]] * len(sims), sims] * n_seeds)
    curves = batch.train(n_iter, N, b, alpha, nu, n_rollout, costs="reference")
    out = {"theta_sim": theta_sim, "seeds": seeds, "batch": batch, "members": members}
    for k, kind in enumerate(("unsafe", "safe", "ensemble")):
        out[f"{kind}_returns"] = curves[k::3]
        out[f"{kind}_costs"] = batch.costs[k::3]
        out[f"{kind}_violations"] = batch.real_violations[k::3]
        out[f"mean_{kind}_returns"] = np.mean(out[f"{kind}_returns"], axis=0)
        out[f"mean_{kind}_costs"] = np.mean(out[f"{kind}_costs"], axis=0)
        out[f"std_{kind}_returns"] = np.std(out[f"{kind}_returns"], axis=0)
    out["member_refusals"] = batch.member_refusals[2::3]
    out["worst_margin"] = float(sim_thresh - batch.worst_max[2::3].max())    # worst_max is 0 where nothing was admitted
    return out


def figure_path(path, epsilon, thresh, n_seeds):
    return f"{path}safe_ars_swimmer_epsilon={epsilon}_thresh={thresh}_n_seeds={n_seeds}.png"


def save_figure(out, thresh, n_iter, n_rollout, save_path):
    """The script's 2 x 2 figure (costs above, returns below; without / with safe exploration), Agg backend, no show.
    Returns False when matplotlib cannot be imported."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    steps = 2 * n_iter * n_rollout
    fig, ax = plt.subplots(2, 2, figsize=(10, 10), sharey="row")
    c_t, r_t = np.linspace(0, steps, steps), np.linspace(0, steps, n_iter)
    for col, (kind, title) in enumerate((("unsafe", "without"), ("safe", "with"))):
        ax[0, col].plot(c_t, out[f"mean_{kind}_costs"])
        ax[0, col].plot(c_t, np.full(steps, thresh), color="k")
        ax[0, col].set_title(f"State cost, {title} Safe Exploration")
        mean, std = out[f"mean_{kind}_returns"], out[f"std_{kind}_returns"]
        ax[1, col].plot(r_t, mean, color="#CC4F1B")
        ax[1, col].fill_between(r_t, mean - std, mean + std, alpha=0.5, edgecolor="#CC4F1B", facecolor="#FF9848")
        ax[1, col].set_xlabel("Timesteps")
        ax[1, col].set_title(f"Return, {title} Safe Exploration")
    ax[0, 0].set_ylabel("Cost")
    ax[1, 0].set_ylabel("Returns (mean of each iteration)")
    fig.savefig(save_path)
    plt.close(fig)
    return True


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--epsilon", help="precision of parameter estimation", type=float)
    parser.add_argument("--thresh", help="safety threshold: the state cost should never be higher", type=float)
    parser.add_argument("--n_iter", help="number of ARS training iterations", type=int)
    parser.add_argument("--n_rollout", help="length of one rollout", type=int)
    parser.add_argument("--N", help="number of policy perturbations sampled", type=int)
    parser.add_argument("--b", help="number of perturbations used for the policy update", type=int)
    parser.add_argument("--alpha", help="step size", type=float)
    parser.add_argument("--nu", help="perturbations' standard deviation", type=float)
    parser.add_argument("--path", help="directory for saving the results graph", type=str)
    parser.add_argument("--n_seeds", help="number of random seeds", type=int)
    args = parser.parse_args(argv)
    missing = [k for k, v in vars(args).items() if v is None]
    if missing:
        parser.error("missing: " + ", ".join("--" + k for k in missing))
    out = run(args.epsilon, args.thresh, args.n_iter, args.n_rollout, args.N, args.b, args.alpha, args.nu, args.n_seeds)
    print(f"Real world parameter: {list(THETA_REAL)}")
    print(f"Estimated parameter: {out['theta_sim']}")
    for i, seed in enumerate(out["seeds"]):
        print(f"Experience {i}/{args.n_seeds} with random seed {seed}: last mean return basic "
              f"{out['unsafe_returns'][i, -1]}, safe {out['safe_returns'][i, -1]}; real steps over the threshold "
              f"basic {out['unsafe_violations'][i]}, safe {out['safe_violations'][i]}")
    print(f"Length of returns: {out['mean_safe_returns'].shape}")
    print(f"Length of costs: {out['mean_safe_costs'].shape}")
    save_path = figure_path(args.path, args.epsilon, args.thresh, args.n_seeds)
    if save_figure(out, args.thresh, args.n_iter, args.n_rollout, save_path):
        print(f"Done! Graph saved at {save_path}")
    else:
        print(f"Done! matplotlib is not importable: no graph saved at {save_path}")
    return out


if __name__ == "__main__":
    main()
