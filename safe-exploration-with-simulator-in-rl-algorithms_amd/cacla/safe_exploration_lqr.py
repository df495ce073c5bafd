"""The validity of safe exploration with CACLA on easy parameterised LQR: the reference's
cacla/safe_exploration_lqr.py as a function.  The plain agent and the safe agent train from the same seed -- the
same initial state, the same noise -- the first on the real environment alone, the second behind the simulator's gate.

Choose the environments' class (EasyParamLinearQuadReg, BoundedEasyLinearQuadReg, BoundedActionEasyLinearQuadReg or
EasyAffineQuadReg) and the agent that goes with it: "se" (CACLA_LQR_SE_agent), "bounded" (CACLA_Bounded_LQR_SE_agent)
or "affine" (CACLA_AffineQR_SE_agent); the defaults are the reference script's.

With out_dir (None: no file; the reference's "results/cacla/Safe_LQR/...") and matplotlib, the reference's 3 x 2
figure is written there: states, actions and smoothed rewards without and with safe exploration.
"""
import os

import numpy as np

from ..envs.gym_lqr.lqr_env import EasyAffineQuadReg
from .cacla_safe_agent import Constraint
from .lqr import CACLA_LQR_Batch, norm_cost
from .lqr_experiment import _figures
from .window import window_convolution

OPTIMAL_F = np.array([1 - np.sqrt(3), 0])


def compare(lqr_real=None, lqr_sim=None, agent="affine", theta_real=1.0, theta_sim=0.99, n_iter=20000, gamma=1,
            sigma=0.1, alpha=0.0001, seed=8943948, constraint=None, epsilon=None, H=1000, out_dir=None, chunk=2048,
            device="cuda:0"):
    """-> dict with, for "plain" and "safe": (states, actions, rewards) as the single agents return them, F, the
    distance of F to the optimal policy, the smoothed rewards; and the safe agent's admitted, violations."""
    print("Starting experience of Safe Exploration with CACLA on LQR")
    lqr_real = EasyAffineQuadReg(theta_real) if lqr_real is None else lqr_real
    lqr_sim = EasyAffineQuadReg(theta_sim) if lqr_sim is None else lqr_sim
    epsilon = abs(theta_real - theta_sim) if epsilon is None else epsilon
    constraint = Constraint(norm_cost(np.inf), 4, 1) if constraint is None else constraint
    out = {}
    for name, kind in (("plain", "plain"), ("safe", agent)):
        batch = CACLA_LQR_Batch(lqr_real, gamma, alpha, sigma, [seed], sim_envs=lqr_sim, epsilons=epsilon,
                                constraints=constraint, agent=kind, device=device)
        batch.run(n_iter, chunk=chunk)
        states, actions, rewards = batch.arrays_of(0)
        out[name] = dict(states=states, actions=actions, rewards=rewards, F=batch.F[0],
                         distance=float(np.linalg.norm(batch.F[0] - OPTIMAL_F, 2)),
                         smoothed=window_convolution(rewards, H), admitted=int(batch.admitted[0]),
                         violations=int(batch.violations[0]), status=int(batch.status[0]))
        print(batch.F[0])
    print(f"Optimal: {OPTIMAL_F}")
    print(f"CACLA without Safe Exploration: {out['plain']['F']}; distance = {out['plain']['distance']}")
    print(f"CACLA with Safe Exploration: {out['safe']['F']}; distance = {out['safe']['distance']}")
    new = _figures() if out_dir is not None else None
    if new is not None:
        os.makedirs(out_dir, exist_ok=True)
        fig = new(figsize=(10, 10))
        ax = fig.subplots(3, 2)
        fig.subplots_adjust(wspace=0.4, hspace=0.4)
        t = np.linspace(H, n_iter, max(n_iter - H, 0))
        for col, (name, word) in enumerate((("plain", "without"), ("safe", "with"))):
            r = out[name]
            s, a = np.atleast_2d(r["states"]), np.atleast_2d(r["actions"])
            if s.size and s.shape[1] >= 2:
                ax[0, col].scatter(s[:, 0], s[:, 1], c=np.linspace(0, 1, len(s)))
            ax[0, col].set_xlabel("x1")
            ax[0, col].set_ylabel("x2")
            ax[0, col].set_title(f"States, {word} Safe Exploration")
            if a.size:
                ax[1, col].scatter(range(len(a)), a[:, 0], c=np.linspace(0, 1, len(a)))
            ax[1, col].set_xlabel("Timesteps")
            ax[1, col].set_ylabel("Actions")
            ax[1, col].set_title(f"Actions, {word} Safe Exploration")
            ax[2, col].plot(t[n_iter - len(r["rewards"]):], r["smoothed"])
            ax[2, col].set_xlabel("Timesteps")
            ax[2, col].set_ylabel(f"Average of the last {H} rewards")
            ax[2, col].set_title(f"Average rewards, {word} Safe Exploration")
        fig.suptitle(f"Easy parameterized LQR (theta_real={theta_real}, theta_sim={theta_sim})\n"
                     f"CACLA (gamma={round(gamma, 3)}, alpha={alpha}, sigma={sigma})")
        fig.savefig(os.path.join(out_dir, f"1_theta_real={theta_real}_theta_sim={theta_sim}_gamma={round(gamma, 3)}"
                                          f"_alpha={alpha}_sigma={sigma}_rewards.png"))
    return out
