"""Many Basic_ARS / Safe_ARS agents (safe_ars/ars.py) trained in lock-step: what safe_ars/experiment.py runs one after
the other -- per seed a basic agent, then a safe one from the same seed -- as ONE batch.

`Basic_ARS.train` here trains one agent at a time, perturbs the 2N policies in NumPy, copies the whole [H, d, 2N]
trajectory back every iteration and sorts and updates in NumPy.  The experiment uses those states as cost(state)
only.  ARSBatch runs an iteration of ALL agents as one host-to-device copy of their deltas, one rollout launch
(sw_safe_ars_rollouts_multi_f64: perturbation in the prologue, the per-step simulator gate in the loop for the gated
agents, one cost value per rollout and step instead of a trajectory) and one update launch (sw_ars_update_multi_f64
with top_b = b: Basic_ARS's rule).  Returns, status and counts stay on the device and are read every READ_EVERY
iterations and at the end.

Every agent keeps the random stream of its seed (ars.agent_batch.SeedStreams): the deltas np.random.seed(seed) followed
by train() would draw.  Two agents with the same seed draw the same deltas, as the reference's pair does.  NumPy's
global generator is never touched.
"""
import numpy as np
import torch

from .. import kernels
from .._lib import SwParams, kernel_flags, require_gpu
from ..ars.agent_batch import READ_EVERY, SeedStreams
from .ars import NativeCost


def _per_agent(value, A, name, dtype=np.float64):
    out = np.asarray(value, dtype=dtype)
    if out.ndim == 0:
        return np.full(A, out, dtype=dtype)
    if out.shape != (A,):
        raise ValueError(f"{name}: expected a scalar or {A} values, got shape {out.shape}")
    return out.copy()


class ARSBatch(object):
    """A agents on one real swimmer.  seeds: one per agent.  gated: per agent (or one for all) -- False: Basic_ARS,
    True: Safe_ARS with `cost`, real_thresh, sim_thresh and sim_envs, each per agent or one for all.  sim_envs may be
    None when no agent is gated.  `rollout_kernel` as Safe_ARS's ("auto" | "lane" | "quad")."""

    def __init__(self, real_env, seeds, gated, cost, real_thresh, sim_thresh=None, sim_envs=None, *, device=None,
                 rollout_kernel="auto"):
        seeds = list(seeds)
        if not seeds:
            raise ValueError("ARSBatch needs at least one seed")
        if not isinstance(cost, NativeCost):
            raise TypeError("ARSBatch needs a NativeCost (AbsObs / MaxAbsThetaDot): the cost is evaluated inside the "
                            "rollout kernel; any other callable trains agent by agent on the lock-step classes "
                            "Basic_ARS / Safe_ARS")
        self.A = A = len(seeds)
        self.seeds = seeds
        self.gated = _per_agent(gated, A, "gated", dtype=bool)
        self.cost = cost
        self.real_thresh = _per_agent(real_thresh, A, "real_thresh")
        if self.gated.any() and (sim_thresh is None or sim_envs is None):
            raise ValueError("gated agents need sim_thresh and sim_envs")
        self.sim_thresh = _per_agent(0.0 if sim_thresh is None else sim_thresh, A, "sim_thresh")
        n = real_env.n
        if sim_envs is None or not isinstance(sim_envs, (list, tuple)):
            sim_envs = [sim_envs] * A
        if len(sim_envs) != A:
            raise ValueError(f"sim_envs: expected one simulator or {A}, got {len(sim_envs)}")
        sim = np.empty((A, 3))
        for a, env in enumerate(sim_envs):
            if env is None:
                if self.gated[a]:
                    raise ValueError(f"sim_envs[{a}]: a gated agent needs a simulator")
                env = real_env                                  # never read for an ungated agent
            if env.n != n or env.h != real_env.h or not np.array_equal(env.direction, real_env.direction):
                raise ValueError(f"sim_envs[{a}]: n, h and the direction must be the real swimmer's")
            sim[a] = env.l_i, env.m_i, env.k
        self.sim = sim
        self.m, self.d = n - 1, 2 * n + 2
        self.params = SwParams.make(n, real_env.l_i, real_env.m_i, real_env.k, real_env.h, real_env.direction,
                                    flags=kernel_flags(rollout_kernel))
        self.device = torch.device(getattr(real_env, "device", "cuda:0") if device is None else device)
        self.policy = np.zeros((A, self.m, self.d))

    def train(self, n_iter, N, b, alpha, nu, H, costs="reference"):
        """safe_ars/ars.py:67-100 for every agent, from the zero policy.  costs: "reference" keeps the cost trace of
        the rollouts the reference script indexes (the first 2 n_iter of all n_iter * 2N, experiment.py:81-82) as
        self.costs [A, 2 n_iter H]; "all" every rollout's as [A, n_iter * 2N, H]; None: none.  Sets policy [A, m, d],
        curves [A, n_iter], cost_max / first_refused [A, n_iter * 2N], real_violations / status [A] (status: the OR of
        the agent's rollouts' status bits) and returns the curves."""
        if costs not in ("reference", "all", None):
            raise ValueError('costs must be "reference", "all" or None')
        n_iter, N, b, H = int(n_iter), int(N), int(b), int(H)
        if n_iter < 1 or N < 1 or b < 1 or H < 0:
            raise ValueError("train needs n_iter >= 1, N >= 1, b >= 1 and H >= 0")
        require_gpu()
        A, dev, R = self.A, self.device, 2 * N
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        policy = torch.zeros((A, self.m, self.d), **f64)
        gated = torch.as_tensor(self.gated.astype(np.int32), device=dev)
        sim, sim_thr, real_thr = (torch.as_tensor(x, device=dev) for x in (self.sim, self.sim_thresh, self.real_thresh))
        deltas = torch.empty((A, N, self.m, self.d), **f64)
        host = [torch.empty((A, N, self.m, self.d), dtype=torch.float64).pin_memory() for _ in range(4)]
        copied = [None] * len(host)
        streams = SeedStreams(self.seeds)
        rows = min(READ_EVERY, n_iter)
        ret_hist, cmax_hist = torch.zeros((rows, A, R), **f64), torch.zeros((rows, A, R), **f64)
        ref_hist, viol_hist, stat_hist = (torch.zeros((rows, A, R), **i32) for _ in range(3))
        # cost traces [H, A, 2N] per iteration: "reference" keeps the iterations that hold the script's 2 n_iter
        # rollouts, "all" a ring of READ_EVERY iterations drained with the other reads
        n_traced = 0 if costs is None else (n_iter if costs == "all" else -(-2 * n_iter // R))
        trace = torch.zeros((min(n_traced, rows) if costs == "all" else n_traced, H, A, R), **f64) if n_traced else None
        self.curves = np.empty((A, n_iter))
        self.cost_max = np.empty((A, n_iter * R))
        self.first_refused = np.empty((A, n_iter * R), dtype=np.int32)
        self.real_violations = np.zeros(A, dtype=np.int64)
        self.status = np.zeros(A, dtype=np.int32)
        all_costs = np.empty((A, n_iter * R, H)) if costs == "all" else None

        def read(pending):
            idx = torch.as_tensor([row for _, row in pending], device=dev)
            got = [t.index_select(0, idx).cpu().numpy() for t in (ret_hist, cmax_hist, ref_hist, viol_hist, stat_hist)]
            tr = trace.index_select(0, idx).cpu().numpy() if costs == "all" else None
            for k, (it, _) in enumerate(pending):
                rets, cmax, ref, viol, stat = (g[k] for g in got)
                self.curves[:, it] = [np.mean(rets[a]) for a in range(A)]
                self.cost_max[:, it * R:(it + 1) * R] = cmax
                self.first_refused[:, it * R:(it + 1) * R] = ref
                self.real_violations += viol.sum(axis=1)
                self.status |= np.bitwise_or.reduce(stat, axis=1)
                if tr is not None:
                    all_costs[:, it * R:(it + 1) * R] = tr[k].transpose(1, 2, 0)     # [H, A, 2N] -> [A, 2N, H]

        pending = []
        for it in range(n_iter):
            k, row = it % len(host), it % rows
            if copied[k] is not None:
                copied[k].synchronize()          # the copy that last read this host buffer is done
            streams.fill(host[k].numpy())
            deltas.copy_(host[k], non_blocking=True)
            if copied[k] is None:
                copied[k] = torch.cuda.Event()
            copied[k].record()
            tr = None
            if it < n_traced:
                tr = trace[row if costs == "all" else it]
            kernels.safe_ars_rollouts_multi(self.params, H, policy, deltas, nu, gated, sim, sim_thr, real_thr,
                                            self.cost.kind, self.cost.index, returns=ret_hist[row], cost_trace=tr,
                                            cost_max=cmax_hist[row], first_refused=ref_hist[row],
                                            violations=viol_hist[row], status=stat_hist[row])
            kernels.ars_update_multi(self.params, ret_hist[row], deltas, policy, alpha, float(b), top_b=b)
            pending.append((it, row))
            if len(pending) == rows or it == n_iter - 1:
                read(pending)
                pending = []
        self.policy = policy.cpu().numpy()
        self.costs = all_costs
        if costs == "reference":
            # rollout i = it * 2N + r of the script's first 2 n_iter, its H costs in a row
            tr = trace.cpu().numpy().transpose(2, 0, 3, 1).reshape(A, n_traced * R, H)    # [A, it * 2N + r, H]
            self.costs = np.ascontiguousarray(tr[:, :2 * n_iter]).reshape(A, 2 * n_iter * H)
        return self.curves
