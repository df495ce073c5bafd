"""Several independent ARS agents advanced in lock-step: what `Experiment.plot(n_seed, ...)` trains
(ars/experiment.py:61-72 starts one Ray actor per seed, each an ARSAgent seeded with its index).

With the reference's own configurations (N = 1 or a handful of directions) an agent's iteration is a
rollout launch that fills a fraction of one wave, an update and a host round trip; the launches of
different seeds do not depend on each other.  ARSAgentBatch runs them as ONE rollout launch
(sw_ars_rollouts_multi_f64) and ONE update launch (sw_ars_update_multi_f64) per iteration for all seeds,
behind one host-to-device copy of all their deltas.  No collective.

Every agent keeps what makes it the agent of its seed:
  * its own random stream -- the MT19937 state np.random.seed(seed) would give NumPy's global generator
    (ars_agent.py:94-95), held per agent and advanced by the native generator (sw_mt19937_uniform_pm1), so
    agent s draws exactly the deltas ARSAgent(seed=s) draws; NumPy's global generator is never touched;
  * its own policy, V2 running statistics, mean and inv_std.
Per agent the kernels run the instructions of the single-agent kernels, so agent s's returns, policy and
statistics are, bit for bit, those of ARSAgent(seed=s, full_covariance=False).

Not here (each raises at construction): safe=True (the simulator gate is not batched: it needs per-agent
simulator constants and thresholds), more than one rank, trajectory capture / the trajectory store.
"""
import ctypes

import numpy as np
import torch
import torch.distributed as dist

from .. import kernels
from .._lib import SwParams, SwimmerHipError, check, kernel_flags, load, require_gpu

SLOT_GRANULE = 16        # rollout slots per workgroup of the segment-per-lane forms = one V2 moment row
SLOT_GRANULE_LANE = 64   # ... of the lane form
READ_EVERY = 10          # iterations between two reads of the curve (where the reference prints, ars_agent.py:203)


def slot_layout(n_agent, n_roll, granule=SLOT_GRANULE):
    """The rollout slots of a multi-agent launch (sw_ars_rollouts_multi_f64): every agent gets
    granule * ceil(n_roll / granule) consecutive slots, i.e. whole workgroups and whole 16-rollout moment rows.
    Returns (agent, local, valid), one entry per slot: the agent the slot belongs to, the agent's rollout it
    computes, and whether it writes anything -- an idle slot (valid False) recomputes the agent's LAST rollout
    and stores nothing, as the tail of a single-agent launch does."""
    n_agent, n_roll, granule = int(n_agent), int(n_roll), int(granule)
    if n_agent < 1 or n_roll < 1 or granule < 1:
        raise ValueError("slot_layout needs n_agent >= 1, n_roll >= 1 and granule >= 1")
    per_agent = granule * -(-n_roll // granule)
    slot = np.arange(n_agent * per_agent, dtype=np.int64)
    agent, raw = slot // per_agent, slot % per_agent
    valid = raw < n_roll
    return agent, np.where(valid, raw, n_roll - 1), valid


class SeedStreams(object):
    """One legacy MT19937 stream per seed, each in the state np.random.seed(seed) leaves NumPy's global
    generator in; `fill(out)` writes 2 * rand - 1 of stream s into out[s] and advances that stream only."""

    def __init__(self, seeds):
        self.seeds = list(seeds)
        self._keys, self._pos = [], []
        for seed in self.seeds:
            kind, key, pos, _, _ = np.random.RandomState(seed).get_state()
            assert kind == "MT19937"
            self._keys.append(np.ascontiguousarray(key, dtype=np.uint32).copy())
            self._pos.append(ctypes.c_int32(int(pos)))
        self._fn = load().sw_mt19937_uniform_pm1
        self._state = [(key.ctypes.data_as(ctypes.c_void_p), ctypes.byref(pos))
                       for key, pos in zip(self._keys, self._pos)]
        self._bound = {}      # per destination buffer: the calls' argument tuples, converted once

    def fill(self, out):
        """out: C-contiguous float64 array [len(seeds), ...]."""
        if out.dtype != np.float64 or not out.flags.c_contiguous or out.shape[0] != len(self.seeds):
            raise SwimmerHipError("SeedStreams.fill needs a C-contiguous float64 array with one row per seed")
        base, stride, per = out.ctypes.data, out.strides[0], out[0].size
        calls = self._bound.get((base, stride, per))
        if calls is None:
            if len(self._bound) >= 16:
                self._bound.clear()
            calls = self._bound[(base, stride, per)] = [
                (key, pos, per, ctypes.c_void_p(base + s * stride)) for s, (key, pos) in enumerate(self._state)]
        fn = self._fn
        for args in calls:
            rc = fn(*args)
            if rc:
                check(rc, "sw_mt19937_uniform_pm1")
        return out


class ARSAgentBatch(object):

    def __init__(self, real_env_param, agent_param, seeds, *, device=None, top_b=0, rollout_kernel="auto",
                 record_trajectories=False):
        seeds = list(seeds)
        if not seeds:
            raise ValueError("ARSAgentBatch needs at least one seed")
        if agent_param.safe:
            raise NotImplementedError("ARSAgentBatch: safe=True is not batched (the simulator gate needs per-agent "
                                      "simulator constants and thresholds); train safe agents one by one with ARSAgent")
        if record_trajectories:
            raise NotImplementedError("ARSAgentBatch stores no trajectories (no capture in the multi-agent kernels, "
                                      "no Database); use ARSAgent(record_trajectories=True)")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("ARSAgentBatch runs on one rank: a batch is not sharded")
        flags = kernel_flags(rollout_kernel)
        if int(top_b) < 0:
            raise ValueError("top_b must be >= 0")
        n = real_env_param.n
        self.m, self.d = n - 1, 2 * n + 2
        if agent_param.initial_w == 'Zero':
            start = np.zeros((self.m, self.d))
        else:
            start = np.load(agent_param.initial_w)
            if start.shape != (self.m, self.d):
                raise ValueError(f"initial_w: policy of shape {start.shape}, expected {(self.m, self.d)}")
        require_gpu()
        self.device = torch.device("cuda:0" if device is None else device)
        self.seeds = seeds
        self.S = S = len(seeds)
        self.real_env_param, self.agent_param = real_env_param, agent_param
        self.top_b = int(top_b)
        self.safe = False
        self.v2 = not agent_param.V1
        self.params = SwParams.make(n, real_env_param.l_i, real_env_param.m_i, real_env_param.k,
                                    real_env_param.h, (1.0, 0.0), flags=flags)
        N = agent_param.N
        f64 = dict(dtype=torch.float64, device=self.device)
        start = np.ascontiguousarray(start, dtype=np.float64)
        self._policy = torch.as_tensor(np.broadcast_to(start, (S,) + start.shape).copy(), device=self.device)
        self._mean = torch.zeros((S, self.d), **f64) if self.v2 else None
        self._inv_std = torch.ones((S, self.d), **f64) if self.v2 else None
        self._running = torch.zeros((S, 1 + 2 * self.d), **f64) if self.v2 else None
        self._moments = (torch.zeros((S, kernels.moments_blocks(2 * N), 2 * self.d), **f64) if self.v2 else None)
        self._sigma = torch.zeros(S, **f64)
        self.n_saved_states = 0
        self._it = 0
        # returns and status of the last READ_EVERY iterations stay on the device: the rollout launch of
        # iteration j writes row j mod READ_EVERY directly, the host reads the rows in one go
        self._ret_hist = torch.zeros((READ_EVERY, S, 2 * N), **f64)
        self._status_hist = torch.zeros((READ_EVERY, S, 2 * N), dtype=torch.int32, device=self.device)
        # deltas: drawn on the host into a small ring of pinned buffers (the event says when the copy that read
        # a buffer is done), copied with ONE host-to-device copy per iteration
        self._streams = SeedStreams(seeds)
        self._deltas = torch.empty((S, N, self.m, self.d), **f64)
        self._host = [torch.empty((S, N, self.m, self.d), dtype=torch.float64).pin_memory() for _ in range(4)]
        self._host_np = [t.numpy() for t in self._host]
        self._copied = [None] * len(self._host)

    # ---- attributes, as ARSAgent's with a leading agent axis ---------------------------------
    @property
    def policy(self):
        return self._policy.cpu().numpy()

    @policy.setter
    def policy(self, value):
        """[S, m, d], or one [m, d] policy for every agent."""
        value = np.broadcast_to(np.asarray(value, dtype=np.float64), (self.S, self.m, self.d)).copy()
        self._policy.copy_(torch.as_tensor(value))

    @property
    def mean(self):
        return None if not self.v2 else self._mean.cpu().numpy()

    @property
    def covariance(self):
        """[S, d, d]: per agent what ARSAgent(full_covariance=False).covariance returns -- the diagonal matrix of
        the V2 running variances (ddof = 1), the identity before the first iteration; None for V1."""
        if not self.v2:
            return None
        if self.n_saved_states == 0:
            return np.stack([np.identity(self.d)] * self.S)
        return np.stack([np.diag(row ** -2.0) for row in self._inv_std.cpu().numpy()])

    # ---- one iteration -----------------------------------------------------------------------
    def run_iteration_async(self, deltas=None):
        """One ARS iteration of every agent without synchronising the host: one copy of the deltas, one rollout
        launch, one update launch.  deltas: None (every agent draws from its own stream) or [S, N, m, d].
        Returns the row of the device-side history this iteration's returns and status go to."""
        ap = self.agent_param
        k = self._it % len(self._host)
        row = self._it % READ_EVERY
        self._it += 1
        if self._copied[k] is not None:
            self._copied[k].synchronize()       # the copy that last read this host buffer is done
        if deltas is None:
            self._streams.fill(self._host_np[k])
        else:
            self._host_np[k][...] = deltas
        self._deltas.copy_(self._host[k], non_blocking=True)
        if self._copied[k] is None:
            self._copied[k] = torch.cuda.Event()
        self._copied[k].record()
        returns = self._ret_hist[row]
        kernels.ars_rollouts_multi(self.params, ap.H, self._policy, self._deltas, ap.nu, self._mean, self._inv_std,
                                   returns=returns, moments=self._moments, status=self._status_hist[row])
        n_new = 2 * ap.N * ap.H
        kernels.ars_update_multi(self.params, returns, self._deltas, self._policy, ap.alpha, ap.b, self.top_b,
                                 moments=self._moments, running=self._running, n_new_states=n_new,
                                 mean=self._mean, inv_std=self._inv_std, sigma_out=self._sigma)
        if self.v2:
            self.n_saved_states += n_new
        return row

    def _read(self, rows):
        """Host copies of the history rows `rows` (returns [len(rows), S, 2N]); raises LinAlgError naming the seeds
        with a failed rollout in any of them."""
        idx = torch.as_tensor(rows, device=self.device)
        rets = self._ret_hist.index_select(0, idx).cpu().numpy()
        status = self._status_hist.index_select(0, idx).cpu().numpy()
        bad = np.flatnonzero((status != 0).any(axis=(0, 2)))
        if bad.size:
            raise np.linalg.LinAlgError("Singular matrix / non-finite state in a rollout of seed(s) "
                                        + ", ".join(str(self.seeds[s]) for s in bad))
        return rets

    def runOneIteration(self):
        """One whole iteration of every agent (ars_agent.py:132-185); returns the [S][2N] returns."""
        return self._read([self.run_iteration_async()])[0]

    def runTraining(self, save_data_path=None, save_policy_path=None):
        """1 warm-up iteration + n_iter iterations of every agent; returns the [S][n_iter + 1] curves, the mean of
        an iteration's 2N returns each (ars_agent.py:187-220).  The host waits for the device only every
        READ_EVERY iterations and at the end.  save_policy_path: the policy of the LAST seed is saved -- in the
        reference every seed's actor writes the same path and the last writer wins."""
        if save_data_path is not None:
            raise NotImplementedError("ARSAgentBatch stores no trajectories: save_data_path needs ARSAgent")
        ap, ep = self.agent_param, self.real_env_param
        curves = np.empty((self.S, ap.n_iter + 1))
        pending = []                                    # (iteration, history row) not read yet
        for j in range(ap.n_iter + 1):
            pending.append((j, self.run_iteration_async()))
            if j % READ_EVERY == 0 or j == ap.n_iter:
                rets = self._read([row for _, row in pending])
                for (it, _), r in zip(pending, rets):
                    curves[:, it] = [np.mean(r[s]) for s in range(self.S)]
                pending = []
                if j % READ_EVERY == 0 and j > 0:
                    variant = "V1" if ap.V1 else "V2"
                    print(f"[seeds {self.seeds[0]}..{self.seeds[-1]}] ARS {variant} n={ep.n} N={ap.N} b={ap.b} "
                          f"alpha={ap.alpha} nu={ap.nu} h={ep.h} l_i={ep.l_i} m_i={ep.m_i} | iteration "
                          f"{j}/{ap.n_iter}: mean return over the seeds {np.mean(curves[:, j])}")
        if save_policy_path is not None:
            np.save(save_policy_path, self.policy[-1])
        return curves
