"""Solving LQR with CACLA, without safe exploration, over a range of step sizes: the reference's
cacla/lqr_experiment.py as a function.  Where the reference trains one agent per step size one after the other, all
of them are ONE CACLA_LQR_Batch: one launch per chunk of steps.

Seeds: the reference seeds nothing; here the agent of alphas[k] is seeded seeds[k] (default k), so a curve can be
reproduced with CACLA_LQR_agent after np.random.seed(seeds[k]).

Files, under out_dir (None: no files; the reference's "results/cacla/LQR/"), when matplotlib imports: per step size
`2_gamma=<round(gamma, 3)>_alpha=<alpha>_sigma=<sigma>.png`, the smoothed learning curve, and `distance.png`, the
distance of the learnt policy to the optimal one against the step size (the figure the reference shows).
"""
import os

import numpy as np

from ..envs.gym_lqr.lqr_env import LinearQuadReg
from .lqr import CACLA_LQR_Batch
from .window import window_convolution

ALPHAS = (0.1, 0.03, 0.01, 0.003, 0.001, 0.0003, 0.0001, 0.00003, 0.00001)
OPTIMAL_F = np.array([[1 - np.sqrt(3), 0]])      # of lqr_2()


def lqr_1():
    """The reference's instance 1: everything 1 x 1 and 1."""
    return LinearQuadReg(np.ones((1, 1)), np.ones((1, 1)), np.ones((1, 1)), np.ones((1, 1)))


def lqr_2():
    """The reference's instance 2, the one its sweep runs on."""
    return LinearQuadReg(np.array([[0, 1], [1, 0]]), np.array([[0], [1]]), np.array([[1, 0], [0, 1]]), np.array([[1]]))


def _figures():
    try:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
    except ImportError:
        return None

    def new(**kw):
        fig = Figure(**kw)
        FigureCanvasAgg(fig)
        return fig
    return new


def sweep(env=None, alphas=ALPHAS, n_iter=200000, gamma=1, sigma=0.1, H=1000, seeds=None, optimal_F=None,
          out_dir=None, chunk=2048, device="cuda:0"):
    """-> dict: alphas, distance [len(alphas)] (||F - optimal_F||_2 after n_iter steps), F [len(alphas), n_ac, n_obs],
    curves (window_convolution(rewards, H) per step size), t (the curves' abscissa), status and actor_updates."""
    env = lqr_2() if env is None else env
    optimal_F = OPTIMAL_F if optimal_F is None else np.asarray(optimal_F)
    alphas = list(alphas)
    seeds = list(range(len(alphas))) if seeds is None else list(seeds)
    batch = CACLA_LQR_Batch(env, gamma, alphas, sigma, seeds, agent="plain", device=device)
    rewards = batch.run(n_iter, chunk=chunk, record=("rewards",))["rewards"]
    distance = [float(np.linalg.norm(F - optimal_F)) for F in batch.F]
    curves = [window_convolution(r, H) for r in rewards]
    t = np.linspace(H, n_iter, max(n_iter - H, 0))
    for F in batch.F:
        print(F)
    new = _figures() if out_dir is not None else None
    if new is not None:
        os.makedirs(out_dir, exist_ok=True)
        for alpha, curve in zip(alphas, curves):
            fig = new()
            axes = fig.add_subplot(111)
            axes.plot(t, curve, label=f"gamma={round(gamma, 3)}, alpha={alpha}, sigma={sigma}")
            axes.legend()
            axes.set_xlabel("Timesteps")
            axes.set_ylabel(f"Average of the last {H} rewards")
            axes.set_title("CACLA on LQR learning curve")
            fig.savefig(os.path.join(out_dir, f"2_gamma={round(gamma, 3)}_alpha={alpha}_sigma={sigma}.png"))
        fig = new()
        axes = fig.add_subplot(111)
        axes.semilogx(alphas, distance)
        axes.set_xlabel("Backpropagation step size")
        axes.set_ylabel("||F - optimal_F||_2")
        axes.grid()
        axes.set_title(f"LQR: distance of the policy after {n_iter} iterations to the optimal one, "
                       "for different backprop step size")
        fig.savefig(os.path.join(out_dir, "distance.png"))
    return dict(alphas=alphas, distance=distance, F=batch.F, curves=curves, t=t, status=batch.status,
                actor_updates=batch.actor_updates)
