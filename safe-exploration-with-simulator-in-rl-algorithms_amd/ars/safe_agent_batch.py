"""Several independent SAFE ARS agents advanced in lock-step: what the reference's ars/safe_exploration.py trains
(one Ray actor per (A, epsilon, seed), each an ARSAgent with safe=True and a simulator of its own).

ARSAgent(safe=True) runs an iteration as a gate launch, a blocking device->host read of the admit flags, then the
real rollouts and the update over the k admitted directions.  SafeARSAgentBatch keeps k on the device: one iteration
of ALL agents is one host-to-device copy of their deltas and four launches,

    sw_ars_gate_multi_f64             every agent's 2N simulator rollouts in ITS simulator against ITS threshold
    sw_ars_pack_admitted_f64          flags -> count k, ascending indices, packed deltas (a failed simulator rollout
                                      refuses its direction: nothing unsafe runs before the host has seen the status)
    sw_ars_rollouts_multi_counted_f64 the 2k real rollouts of every agent
    sw_ars_update_multi_counted_f64   the update with n_dir = k, top_b clamped to k; k = 0 leaves the agent untouched

and the host reads nothing until the curve is read every READ_EVERY iterations (counts, admitted indices, returns and
both status arrays of those iterations stay in a device-side history, as ARSAgentBatch's returns do).

Every agent has its own simulator parameters, simulator threshold, safety threshold, MT19937 stream, policy and V2
statistics; per agent the kernels run the instructions of the single-agent kernels, so row a of every result is, bit
for bit, what ARSAgent(safe=True, seed=seeds[a], full_covariance=False) with the same simulator gives -- the
partial-admission rule included (ars_agent.py's docstring: the k admitted directions packed in ascending order,
sigma_R over their 2k returns, the step divided by b, top_b clamped to k, nothing happens when k = 0).

With sim_ensembles ([S][E] EnvParams, the same E for every agent; sim_params is then None) every agent gates in an
ENSEMBLE of simulators (ars/ensemble.py): the first launch becomes sw_ars_gate_ensemble_f64 -- the members' gates and
the fold, two launches behind one call -- whose admit flags and folded status have the layout the pack reads, so the
other three launches are untouched and the host still reads nothing.  The worst simulated returns join the history.
Row a is then ARSAgent(safe=True, seed=seeds[a], sim_ensemble=sim_ensembles[a], full_covariance=False), bit for bit.

Differences from ARSAgent: a real return below the safety threshold is counted in `violations` but not printed (a
sweep holds hundreds of agents); the estimation is the caller's (sim_params: see ars_agent.approximate_env_params); no
trajectory store, no full covariance; one rank.
"""
import numpy as np
import torch
import torch.distributed as dist

from .. import kernels
from .._lib import SwParams, kernel_flags, require_gpu
from .agent_batch import READ_EVERY, SeedStreams
from .ensemble import check_ensemble, sim_rows
from .ensemble_kernels import ars_gate_ensemble


class SafeARSAgentBatch(object):

    def __init__(self, real_env_param, agent_param, seeds, sim_params, sim_thresholds, *, thresholds=None,
                 device=None, top_b=0, rollout_kernel="auto", sim_ensembles=None):
        seeds = list(seeds)
        if not seeds:
            raise ValueError("SafeARSAgentBatch needs at least one seed")
        if not agent_param.safe:
            raise ValueError("SafeARSAgentBatch trains safe agents: agent_param.safe must be True "
                             "(ARSAgentBatch trains the unsafe ones)")
        S = len(seeds)
        if sim_ensembles is not None:
            if sim_params is not None:
                raise ValueError("SafeARSAgentBatch: sim_params (one simulator per agent) or sim_ensembles (several), "
                                 "not both")
            sim_ensembles = [list(ens) for ens in sim_ensembles]
            if len(sim_ensembles) != S:
                raise ValueError(f"SafeARSAgentBatch: {S} seeds need {S} sim_ensembles, got {len(sim_ensembles)}")
            for a, ens in enumerate(sim_ensembles):
                check_ensemble(ens, real_env_param, f"sim_ensembles[{a}]")
                if len(ens) != len(sim_ensembles[0]):
                    raise ValueError(f"sim_ensembles[{a}] holds {len(ens)} simulators, sim_ensembles[0] "
                                     f"{len(sim_ensembles[0])}: the agents of a batch share the ensemble size")
            sim_params = [ens[0] for ens in sim_ensembles]      # what ARSAgent calls estimated_param
        elif sim_params is None:
            raise ValueError("SafeARSAgentBatch needs sim_params or sim_ensembles")
        sim_params = list(sim_params)
        sim_thresholds = [float(t) for t in sim_thresholds]
        if len(sim_params) != S or len(sim_thresholds) != S:
            raise ValueError(f"SafeARSAgentBatch: {S} seeds need {S} sim_params and {S} sim_thresholds, got "
                             f"{len(sim_params)} and {len(sim_thresholds)}")
        if thresholds is None:
            thresholds = [agent_param.threshold] * S
        thresholds = [float(t) for t in thresholds]
        if len(thresholds) != S:
            raise ValueError(f"SafeARSAgentBatch: {S} seeds need {S} thresholds, got {len(thresholds)}")
        for a, sp in enumerate(sim_params):
            if sp.n != real_env_param.n or sp.h != real_env_param.h:
                raise ValueError(f"sim_params[{a}]: n = {sp.n}, h = {sp.h}; the batch's simulators share the real "
                                 f"world's n = {real_env_param.n} and h = {real_env_param.h}")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("SafeARSAgentBatch runs on one rank: a batch is not sharded")
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
        self.seeds, self.S = seeds, S
        self.real_env_param, self.agent_param = real_env_param, agent_param
        self.sim_params, self.sim_thresholds = sim_params, np.array(sim_thresholds)
        self.sim_ensembles = sim_ensembles
        self.thresholds = np.array(thresholds)
        self.top_b = int(top_b)
        self.safe = True
        self.v2 = not agent_param.V1
        # the real world; it also carries n, h, the direction and the flags of every simulator (the gate's `base`)
        self.params = SwParams.make(n, real_env_param.l_i, real_env_param.m_i, real_env_param.k,
                                    real_env_param.h, (1.0, 0.0), flags=flags)
        N = agent_param.N
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self._sim = torch.as_tensor(np.array([[sp.l_i, sp.m_i, sp.k] for sp in sim_params], dtype=np.float64),
                                    device=self.device)
        self._sim_thresh = torch.as_tensor(self.sim_thresholds, device=self.device)
        start = np.ascontiguousarray(start, dtype=np.float64)
        self._policy = torch.as_tensor(np.broadcast_to(start, (S,) + start.shape).copy(), device=self.device)
        self._mean = torch.zeros((S, self.d), **f64) if self.v2 else None
        self._inv_std = torch.ones((S, self.d), **f64) if self.v2 else None
        self._running = torch.zeros((S, 1 + 2 * self.d), **f64) if self.v2 else None
        self._moments = (torch.zeros((S, kernels.moments_blocks(2 * N), 2 * self.d), **f64) if self.v2 else None)
        self._sigma = torch.zeros(S, **f64)
        self.violations = np.zeros(S, dtype=np.int64)       # real returns below the agent's threshold so far
        self.last_admitted = [np.zeros(0, dtype=np.int64) for _ in range(S)]
        self.last_returns = [np.zeros(0) for _ in range(S)]
        self._it = 0
        # what the host wants of the last READ_EVERY iterations stays on the device: the launches of iteration j
        # write row j mod READ_EVERY directly, the host reads the rows in one go
        self._ret_hist = torch.zeros((READ_EVERY, S, 2 * N), **f64)
        self._status_hist = torch.zeros((READ_EVERY, S, 2 * N), **i32)
        self._gate_status_hist = torch.zeros((READ_EVERY, S, 2 * N), **i32)
        self._count_hist = torch.zeros((READ_EVERY, S), **i32)
        self._order_hist = torch.zeros((READ_EVERY, S, N), **i32)
        self._gate_returns = torch.zeros((S, 2 * N), **f64)
        self._admit = torch.zeros((S, N), **i32)
        self.last_worst = [np.zeros(0) for _ in range(S)]
        self.min_admitted_worst = np.full(S, np.inf)        # over every admitted direction of every iteration read
        if sim_ensembles is not None:
            E = len(sim_ensembles[0])
            self._ens_sim = torch.as_tensor(np.stack([sim_rows(ens) for ens in sim_ensembles]), device=self.device)
            self._worst_hist = torch.zeros((READ_EVERY, S, 2 * N), **f64)
            self._ens_returns = torch.zeros((S, E, 2 * N), **f64)
            self._ens_status = torch.zeros((S, E, 2 * N), **i32)
            self._ens_admit = torch.zeros((S, E, N), **i32)
        # deltas: drawn on the host into a small ring of pinned buffers, ONE host-to-device copy per iteration
        self._streams = SeedStreams(seeds)
        self._deltas = torch.empty((S, N, self.m, self.d), **f64)
        self._packed = torch.zeros((S, N, self.m, self.d), **f64)
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
        the V2 running variances (ddof = 1), the identity while the agent has admitted nothing; None for V1."""
        if not self.v2:
            return None
        seen = self._running[:, 0].cpu().numpy()
        inv_std = self._inv_std.cpu().numpy()
        return np.stack([np.diag(row ** -2.0) if cnt > 0 else np.identity(self.d)
                         for row, cnt in zip(inv_std, seen)])

    # ---- one iteration -----------------------------------------------------------------------
    def run_iteration_async(self, deltas=None):
        """One safe iteration of every agent without synchronising the host: the copy of the deltas, then gate,
        pack, counted rollouts, counted update.  deltas: None (every agent draws from its own stream) or
        [S, N, m, d].  Returns the row of the device-side history this iteration's results go to."""
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
        gate_status, count = self._gate_status_hist[row], self._count_hist[row]
        returns = self._ret_hist[row]
        if self.sim_ensembles is not None:
            ars_gate_ensemble(self.params, ap.H, self._policy, self._deltas, ap.nu, self._ens_sim, self._sim_thresh,
                              self._mean, self._inv_std, admit=self._admit, worst=self._worst_hist[row],
                              status=gate_status, member_returns=self._ens_returns, member_status=self._ens_status,
                              member_admit=self._ens_admit)
        else:
            kernels.ars_gate_multi(self.params, ap.H, self._policy, self._deltas, ap.nu, self._sim, self._sim_thresh,
                                   self._mean, self._inv_std, returns=self._gate_returns, status=gate_status,
                                   admit=self._admit)
        kernels.ars_pack_admitted(self.params, self._admit, self._deltas, status=gate_status, count=count,
                                  order=self._order_hist[row], packed=self._packed)
        kernels.ars_rollouts_multi_counted(self.params, ap.H, self._policy, self._packed, ap.nu, count, self._mean,
                                           self._inv_std, returns=returns, moments=self._moments,
                                           status=self._status_hist[row])
        kernels.ars_update_multi_counted(self.params, ap.H, count, returns, self._packed, self._policy, ap.alpha, ap.b,
                                         self.top_b, moments=self._moments, running=self._running, mean=self._mean,
                                         inv_std=self._inv_std, sigma_out=self._sigma)
        return row

    def _read(self, rows):
        """Host copies of the history rows `rows`: a list, per row, of the S agents' 2k returns.  Counts the
        violations, sets last_admitted / last_returns to the last row's, and then raises LinAlgError naming the
        agents with a failed simulator or real rollout in any of the rows."""
        idx = torch.as_tensor(rows, device=self.device)
        rets = self._ret_hist.index_select(0, idx).cpu().numpy()
        status = self._status_hist.index_select(0, idx).cpu().numpy()
        gate_status = self._gate_status_hist.index_select(0, idx).cpu().numpy()
        counts = self._count_hist.index_select(0, idx).cpu().numpy()
        order = self._order_hist.index_select(0, idx).cpu().numpy()
        worst = (self._worst_hist.index_select(0, idx).cpu().numpy() if self.sim_ensembles is not None else None)
        out, bad = [], set()
        for i in range(len(rows)):
            per_agent = []
            for s in range(self.S):
                k = int(counts[i, s])
                r = rets[i, s, :2 * k].copy()
                if gate_status[i, s].any() or status[i, s, :2 * k].any():
                    bad.add(s)
                self.violations[s] += int(np.count_nonzero(r < self.thresholds[s]))
                if worst is not None and k > 0:
                    w = worst[i, s].reshape(-1, 2)[order[i, s, :k]]
                    self.min_admitted_worst[s] = min(self.min_admitted_worst[s], float(w.min()))
                per_agent.append(r)
            out.append(per_agent)
        last = len(rows) - 1
        self.last_admitted = [order[last, s, :int(counts[last, s])].astype(np.int64) for s in range(self.S)]
        self.last_returns = out[last]
        if worst is not None:
            self.last_worst = [worst[last, s].copy() for s in range(self.S)]
        if bad:
            raise np.linalg.LinAlgError("Singular matrix / non-finite state in a simulator or real rollout of "
                                        + ", ".join(f"agent {s} (seed {self.seeds[s]})" for s in sorted(bad)))
        return out

    def runOneIteration(self):
        """One whole safe iteration of every agent (ars_agent.py:132-185); returns S lists: agent a's 2k returns of
        its admitted directions' real rollouts, in order."""
        return [r.tolist() for r in self._read([self.run_iteration_async()])[0]]

    def runTraining(self, save_policy_path=None):
        """1 warm-up iteration + n_iter iterations of every agent; returns the [S][n_iter + 1] curves by ARSAgent's
        rule: the mean of an iteration's 2k returns, the previous value when k = 0, NaN when the warm-up iteration
        is refused (ars_agent.py:187-220).  The host waits for the device only every READ_EVERY iterations and at
        the end.  save_policy_path: the policy of the LAST agent is saved, as ARSAgentBatch does."""
        ap = self.agent_param
        curves = np.empty((self.S, ap.n_iter + 1))
        pending = []                                    # (iteration, history row) not read yet
        for j in range(ap.n_iter + 1):
            pending.append((j, self.run_iteration_async()))
            if j % READ_EVERY == 0 or j == ap.n_iter:
                for (it, _), per_agent in zip(pending, self._read([row for _, row in pending])):
                    for s, r in enumerate(per_agent):
                        if len(r) > 0:
                            curves[s, it] = np.mean(r)
                        else:
                            curves[s, it] = curves[s, it - 1] if it > 0 else np.nan
                pending = []
        if save_policy_path is not None:
            np.save(save_policy_path, self.policy[-1])
        return curves
