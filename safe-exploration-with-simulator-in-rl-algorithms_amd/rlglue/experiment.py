"""The reference's third training program -- SwimmerARSAgent (rlglue/agent/SwimmerAgent.py) driven by
SwimmerExperiment (rlglue/experiment/SwimmerExperiment.cpp) on its native swimmer -- without the three processes and
their sockets: whole runs inside one kernel (kernels.rlglue_ars_run, one agent per lane), many seeds and step sizes per
launch.

What the host does is the agent's random stream and nothing else: the deltas are `np.random.RandomState(seed).rand`
in the agent's order (N matrices at agent_start, N more after every iteration; sample_deltas, SwimmerAgent.py:203-212),
drawn for a chunk of iterations ahead and handed to the launch.  NumPy's global generator is not touched.
"""
import numpy as np
import torch

from .. import _lib
from . import kernels
from .parameters import Parameters

# env-steps per agent and launch, at most.  Measured (scripts/rlglue_probe.py, profiles/rlglue_probe.log): a step of an
# agent's chain takes 0.93-0.98 us at n = 3 and 3.9-4.0 us at n = 6, flat from 1 to 4096 agents, so a full chunk is a
# launch of 1 s resp. 4 s: long enough that the launch's fixed cost and the host's draws vanish (100 iterations of the
# shipped parameters, 3e5 steps: 0.29 s end to end, 0.28 s of it the chain), short enough to stay well clear of any
# launch time limit at n = 8 too.  The probe left the 1e6 of the first draft as it was.
CHUNK_ENV_STEPS = 1_000_000
CHUNK_DELTA_BYTES = 64 << 20     # and never more than this many bytes of deltas per launch (short segments, many
                                 # agents: the draws of 1e6 steps would not fit the device otherwise)


class SwimmerExperimentBatch(object):
    """Many RL-Glue ARS experiments in one launch per chunk of iterations: shared physics, max_u, N, b and H; per-agent
    seed, alpha and nu.  Row a is bit for bit SwimmerExperiment(params with alphas[a], nus[a], seed=seeds[a]).  Never
    raises on a NaN: `status` has the agents' SW_STATUS_* bits."""

    def __init__(self, params: Parameters, seeds, alphas=None, nus=None, device="cuda:0"):
        self.params = p = params.validate()
        self.seeds = list(seeds)
        A = self.n_agent = len(self.seeds)
        if A < 1:
            raise ValueError("need at least one seed")
        alphas = np.full(A, p.alpha) if alphas is None else np.asarray(alphas, dtype=np.float64)
        nus = np.full(A, p.nu) if nus is None else np.asarray(nus, dtype=np.float64)
        if alphas.shape != (A,) or nus.shape != (A,):
            raise ValueError(f"alphas and nus must have one entry per seed ({A})")
        _lib.require_gpu()
        self.device = torch.device(device)
        self.sw_params = _lib.SwParams.make(p.n_seg, p.l_i, p.m_i, p.k, p.h_global, p.direction,
                                            flags=_lib.FLAG_MODEL_TWIN)
        self.m, self.d = self.sw_params.m, self.sw_params.d
        self._rng = [np.random.RandomState(s) for s in self.seeds]
        self._pending = self._draw(1)[0]            # agent_start's sample_deltas: [N, m, d, A]
        self._alpha = _lib.dev_f64(alphas, self.device)
        self._nu = _lib.dev_f64(nus, self.device)
        self._policy = torch.zeros((self.m, self.d, A), dtype=torch.float64, device=self.device)
        self._carry = torch.zeros((self.m + 1, A), dtype=torch.float64, device=self.device)
        self._status = torch.zeros((A,), dtype=torch.int32, device=self.device)
        self.iterations = 0
        self._eval_chunks = [np.empty((0, A))]              # per launch: [c, A] and [c, 2N, A], joined on read
        self._train_chunks = [np.empty((0, 2 * p.N, A))]

    def _draw(self, n_it):
        """The next n_it sample_deltas() of every agent, agent-minor: [n_it, N, m, d, A]."""
        shape = (n_it, self.params.N, self.m, self.d)
        return np.stack([rs.rand(*shape) for rs in self._rng], axis=-1)

    def _chunk_iterations(self):
        p = self.params
        by_steps = CHUNK_ENV_STEPS // ((2 * p.N + 1) * p.H)
        by_bytes = CHUNK_DELTA_BYTES // (8 * p.N * self.m * self.d * self.n_agent)
        return max(1, min(by_steps, by_bytes))

    def run(self, n_it):
        """n_it more iterations; -> their evaluation returns [n_agent, n_it].  Calling again continues the run."""
        n_it = int(n_it)
        if n_it < 0:
            raise ValueError("n_it must be >= 0")
        p, chunk = self.params, self._chunk_iterations()
        done = 0
        while done < n_it:
            c = min(chunk, n_it - done)
            fresh = self._draw(c)                   # the draws after iterations 0 .. c-1 of this chunk
            deltas = np.concatenate([self._pending[None], fresh[:-1]], axis=0)
            self._pending = fresh[-1]               # drawn after the last iteration: the next call's first
            ev, tr = kernels.rlglue_ars_run(self.sw_params, p.max_u, self.iterations, c, p.N, p.b, p.H, self._alpha,
                                            self._nu, _lib.dev_f64(deltas, self.device), self._policy, self._carry,
                                            self._status)
            self._eval_chunks.append(ev.cpu().numpy())
            self._train_chunks.append(tr.cpu().numpy())
            self.iterations += c
            done += c
        return np.ascontiguousarray(self._eval[self.iterations - n_it:].T)

    @property
    def _eval(self):
        if len(self._eval_chunks) > 1:
            self._eval_chunks = [np.concatenate(self._eval_chunks, axis=0)]
        return self._eval_chunks[0]

    @property
    def _train(self):
        if len(self._train_chunks) > 1:
            self._train_chunks = [np.concatenate(self._train_chunks, axis=0)]
        return self._train_chunks[0]

    @property
    def eval_returns(self):
        """[n_agent, iterations]: every evaluation return so far."""
        return np.ascontiguousarray(self._eval.T)

    @property
    def policy(self):
        """[n_agent, m, d]"""
        return np.ascontiguousarray(self._policy.cpu().numpy().transpose(2, 0, 1))

    @property
    def train_returns(self):
        """[n_agent, iterations, 2N]: `rewards` as update_policy saw it."""
        return np.ascontiguousarray(self._train.transpose(2, 0, 1))

    @property
    def status(self):
        """int32 [n_agent]: SW_STATUS_* bits accumulated over the run."""
        return self._status.cpu().numpy()

    def write_results(self, path, agent=0):
        """One agent's evaluation returns in the line format of SwimmerExperiment.cpp:83 (a C++ stream's default
        6 significant digits), which rlglue/plot/show_results.py reads."""
        with open(path, "w") as f:
            for i, r in enumerate(self._eval[:, agent]):
                f.write(f"Reward for one rollout with policy at iteration {i}: {r:g}\n")


class SwimmerExperiment(object):
    """One run of the reference's `./SwimmerExperiment n_it` with `parameters.txt` = params: a batch of one."""

    def __init__(self, params: Parameters, seed=None, device="cuda:0"):
        self.params = params
        self._batch = SwimmerExperimentBatch(params, [seed], device=device)

    def run(self, n_it):
        """n_it more iterations; -> their evaluation returns [n_it].  ValueError where the reference's
        statistics.stdev raises: a return that is not finite."""
        out = self._batch.run(n_it)[0]
        if self.status & _lib.STATUS_NONFINITE:
            raise ValueError(f"a return, a state or the policy is not finite after {self.iterations} iterations "
                             f"(status {self.status}): the reference's statistics.stdev raises on such a run")
        return out

    @property
    def iterations(self):
        return self._batch.iterations

    @property
    def eval_returns(self):
        return self._batch.eval_returns[0]

    @property
    def policy(self):
        return self._batch.policy[0]

    @property
    def train_returns(self):
        return self._batch.train_returns[0]

    @property
    def status(self):
        return int(self._batch.status[0])

    def write_results(self, path):
        self._batch.write_results(path, 0)
