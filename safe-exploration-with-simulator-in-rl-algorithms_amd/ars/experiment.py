"""Learning curves over several seeds: the reference's `Experiment` (ars/experiment.py:13-122), the level every
script of the reference goes through (plot_graph.py, state_range.py, safe_exploration.py, comparison_mujoco.py).

Same constructor, same `plot(n_seed, agent_param, plot_mean=True)`, same result (r_graphs [n_seed][n_iter + 1])
and the same files: `results_path + "array/" + <name>.npy` with the curves, and -- when matplotlib imports --
`results_path + "new/" + <name>.png` and `<name>-average.png`, <name> built as the reference builds it
(experiment.py:44-56, :90-95).  The directories are created when missing.  There is no Ray: where the reference
starts one actor per seed,

  * unsafe agents without a trajectory store train as ONE ARSAgentBatch over seeds 0 .. n_seed - 1: one rollout
    launch and one update launch per iteration for all of them (ars/agent_batch.py);
  * safe=True, a save_data_path or more than one rank take the seeds one after another through ARSAgent with the
    reference's arguments (the simulator gate is not batched, and the batch stores no trajectories).

Both give, row by row, what ARSAgent(seed=s).runTraining() gives.

save_policy_path: in the reference every seed's actor saves to the same path, so the file holds whichever actor
finished last; here it holds the policy of seed n_seed - 1 on both paths.
"""
import os

import numpy as np
import torch.distributed as dist

from .agent_batch import ARSAgentBatch
from .ars_agent import ARSAgent


def describe(real_env_param, agent_param):
    """(environment, ARS): the two comma-separated descriptions the reference prints, puts in the figures' titles
    and builds its file names of (experiment.py:44-56)."""
    ap, ep = agent_param, real_env_param
    variant = ("ARS_V1" if ap.V1 else "ARS_V2") + ("-t" if ap.b < ap.N else "")
    ars = [str(ap.name), variant, f"n_directions={ap.N}", f"deltas_used={ap.b}", f"step_size={ap.alpha}",
           f"delta_std={ap.nu}"]
    env = [str(ep.name), f"n_segments={ep.n}", f"m_i={round(ep.m_i, 2)}", f"l_i={round(ep.l_i, 2)}",
           f"epsilon={round(ep.epsilon, 4)}", f"deltaT={ep.h}"]
    return ", ".join(env), ", ".join(ars)


def file_stem(real_env_param, agent_param):
    """<name> of the files of one plot() call: both descriptions with '-' for ', ' (experiment.py:90-95)."""
    env, ars = describe(real_env_param, agent_param)
    return env.replace(", ", "-") + "-" + ars.replace(", ", "-")


class Experiment(object):

    def __init__(self, real_env_param, results_path="results/gym/", data_path=None, save_data_path=None,
                 save_policy_path=None, guess_param=None, approx_error=None, sim_thresh=None):
        self.real_env_param = real_env_param
        self.results_path = results_path
        self.guess_param = guess_param
        self.approx_error = approx_error
        self.sim_thresh = sim_thresh
        self.save_policy_path = save_policy_path
        self.data_path = data_path
        self.save_data_path = save_data_path

    def batched(self, agent_param):
        """True when plot() trains the seeds as one ARSAgentBatch."""
        one_rank = not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
        return not agent_param.safe and self.save_data_path is None and one_rank

    def train(self, n_seed, agent_param):
        """r_graphs [n_seed][n_iter + 1]: the learning curve of every seed 0 .. n_seed - 1."""
        if n_seed < 1:
            raise ValueError("n_seed must be at least 1")
        if self.batched(agent_param):
            batch = ARSAgentBatch(self.real_env_param, agent_param, range(n_seed))
            return np.array(batch.runTraining(save_policy_path=self.save_policy_path))
        r_graphs = []
        for seed in range(n_seed):
            agent = ARSAgent(self.real_env_param, agent_param, seed=seed, data_path=self.data_path,
                             guess_param=self.guess_param, approx_error=self.approx_error,
                             sim_thresh=self.sim_thresh,
                             record_trajectories=self.save_data_path is not None)
            r_graphs.append(agent.runTraining(save_data_path=self.save_data_path,
                                              save_policy_path=self.save_policy_path))
        return np.array(r_graphs)

    def plot(self, n_seed, agent_param, plot_mean=True):
        # the descriptions first: the approximation branch of a safe agent changes real_env_param
        environment, ars = describe(self.real_env_param, agent_param)
        stem = file_stem(self.real_env_param, agent_param)
        print(f"\n------ {environment} ------")
        print(ars + "\n")
        r_graphs = self.train(n_seed, agent_param)
        os.makedirs(f"{self.results_path}array/", exist_ok=True)
        np.save(f"{self.results_path}array/{stem}", r_graphs)
        self._figures(r_graphs, agent_param, environment, ars, stem, plot_mean)
        return r_graphs

    def _thresholds(self, axes, t, agent_param):
        if not agent_param.safe:
            return
        ep = self.real_env_param
        axes.plot(t, [agent_param.threshold] * len(t), color="black", linewidth=3, label="Safety threshold")
        sim = agent_param.threshold + ep.epsilon * self.sim_thresh.compute_alpha(ep.H)
        axes.plot(t, [sim] * len(t), color="red", linewidth=3, label="Simulator threshold")
        axes.legend()

    def _figures(self, r_graphs, agent_param, environment, ars, stem, plot_mean):
        """The reference's two figures (experiment.py:74-120), drawn with Agg canvases of their own: no pyplot, so
        the caller's backend and figure registry stay as they are.  Skipped when matplotlib does not import."""
        try:
            from matplotlib.backends.backend_agg import FigureCanvasAgg
            from matplotlib.figure import Figure
        except ImportError:
            return
        os.makedirs(f"{self.results_path}new/", exist_ok=True)
        ap = agent_param
        t = np.linspace(0, ap.n_iter * 2 * ap.N * ap.H, ap.n_iter + 1)

        def new_axes():
            fig = Figure(figsize=(10, 8))
            FigureCanvasAgg(fig)
            axes = fig.add_subplot(111)
            axes.set_title(f"------ {environment} ------\n{ars}")
            axes.set_xlabel("Timesteps")
            axes.set_ylabel("Rollouts Average Return")
            return fig, axes

        fig, axes = new_axes()
        for rewards in r_graphs:
            axes.plot(t, rewards)
        self._thresholds(axes, t, ap)
        fig.savefig(f"{self.results_path}new/{stem}.png")
        if plot_mean:
            fig, axes = new_axes()
            mean, std = np.mean(r_graphs, axis=0), np.std(r_graphs, axis=0)
            axes.plot(t, mean, color="#CC4F1B")
            axes.fill_between(t, mean - std, mean + std, alpha=0.5, edgecolor="#CC4F1B", facecolor="#FF9848")
            self._thresholds(axes, t, ap)
            fig.savefig(f"{self.results_path}new/{stem}-average.png")
