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

The gate in an ENSEMBLE of simulators (sim_ensembles; ars/ensemble.py makes them): the look-ahead of every step runs in
every member, up to 64 of them in the lanes of the rollout's group (sw_safe_ars_rollouts_ensemble_f64), and a step is
taken only where every member admits it.  The simulator threshold may then be None: the real threshold itself, the worst
member standing where the script has `thresh - 1`.  Without an ensemble nothing changes, not one launch.
"""
import numpy as np
import torch

from .. import kernels
from .._lib import SwParams, kernel_flags, require_gpu
from ..ars.agent_batch import READ_EVERY, SeedStreams
from .ars import NativeCost
from .ensemble_kernels import safe_ars_rollouts_ensemble

MAX_MEMBERS = 64    # the members of a rollout ride in the lanes of one wave


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
    None when no agent is gated.  `rollout_kernel` as Safe_ARS's ("auto" | "lane" | "quad").

    sim_ensembles: the gate in an ensemble of simulators per agent instead of sim_envs (which is then None) -- one entry
    per agent: None for an ungated agent, else E members, SwimmerEnv or rows (l_i, m_i, k), the same E <= 64 for every
    gated agent (E copies of one simulator: a single-simulator agent in such a batch).  sim_thresh None is then the
    real threshold.  The rollouts run in the one form the ensemble kernel has; rollout_kernel chooses nothing."""

    def __init__(self, real_env, seeds, gated, cost, real_thresh, sim_thresh=None, sim_envs=None, *, device=None,
                 rollout_kernel="auto", sim_ensembles=None):
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
        self.ensemble = sim_ensembles is not None
        if self.ensemble:
            if sim_envs is not None:
                raise ValueError("give sim_envs or sim_ensembles, not both")
            if sim_thresh is None:
                sim_thresh = self.real_thresh
        elif self.gated.any() and (sim_thresh is None or sim_envs is None):
            raise ValueError("gated agents need sim_thresh and sim_envs")
        self.sim_thresh = _per_agent(0.0 if sim_thresh is None else sim_thresh, A, "sim_thresh")
        n = real_env.n
        self.sims = self._ensemble_rows(real_env, sim_ensembles) if self.ensemble else None      # [A, E, 3]
        if sim_envs is None or not isinstance(sim_envs, (list, tuple)):
            sim_envs = [sim_envs] * A
        if len(sim_envs) != A:
            raise ValueError(f"sim_envs: expected one simulator or {A}, got {len(sim_envs)}")
        sim = np.empty((A, 3))
        for a, env in enumerate(sim_envs):
            if env is None:
                if self.gated[a] and not self.ensemble:
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

    def _ensemble_rows(self, real_env, sim_ensembles):
        """[A, E, 3] (l_i, m_i, k); an ungated agent's rows are the real swimmer's and never read."""
        sim_ensembles = list(sim_ensembles)
        if len(sim_ensembles) != self.A:
            raise ValueError(f"sim_ensembles: expected one entry per agent ({self.A}), got {len(sim_ensembles)}")
        rows = [None] * self.A
        for a, members in enumerate(sim_ensembles):
            if members is None:
                if self.gated[a]:
                    raise ValueError(f"sim_ensembles[{a}]: a gated agent needs an ensemble")
                continue
            members = list(members)
            if not 1 <= len(members) <= MAX_MEMBERS:
                raise ValueError(f"sim_ensembles[{a}]: an ensemble has 1 to {MAX_MEMBERS} simulators, "
                                 f"got {len(members)}")
            for e, env in enumerate(members):
                if hasattr(env, "l_i"):
                    if env.n != real_env.n or env.h != real_env.h or \
                            not np.array_equal(env.direction, real_env.direction):
                        raise ValueError(f"sim_ensembles[{a}][{e}]: n, h and the direction must be the real swimmer's")
                    members[e] = (env.l_i, env.m_i, env.k)
            rows[a] = np.asarray(members, dtype=np.float64)
            if rows[a].shape != (len(members), 3):
                raise ValueError(f"sim_ensembles[{a}]: the members are SwimmerEnv or rows (l_i, m_i, k)")
        sizes = {r.shape[0] for r in rows if r is not None}
        if len(sizes) > 1:
            raise ValueError(f"sim_ensembles: every gated agent needs the same number of members, got {sorted(sizes)}; "
                             "per-agent ensemble sizes are not built")
        E = sizes.pop() if sizes else 1
        real = np.tile([real_env.l_i, real_env.m_i, real_env.k], (E, 1))
        return np.stack([real if r is None else r for r in rows])

    def train(self, n_iter, N, b, alpha, nu, H, costs="reference"):
        """safe_ars/ars.py:67-100 for every agent, from the zero policy.  costs: "reference" keeps the cost trace of
        the rollouts the reference script indexes (the first 2 n_iter of all n_iter * 2N, experiment.py:81-82) as
        self.costs [A, 2 n_iter H]; "all" every rollout's as [A, n_iter * 2N, H]; None: none.  Sets policy [A, m, d],
        curves [A, n_iter], cost_max / first_refused [A, n_iter * 2N], real_violations / status [A] (status: the OR of
        the agent's rollouts' status bits) and returns the curves.  With sim_ensembles also worst_max [A, n_iter * 2N]
        (the largest member cost over a rollout's admitted steps; NaN for an ungated agent), refusing_members int64
        [A, n_iter * 2N] (bit e: member e refused the rollout's first refused step) and member_refusals int64 [A, E]
        (the rollouts in which member e was among the refusing ones)."""
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
        hists = [ret_hist, cmax_hist, ref_hist, viol_hist, stat_hist]
        if self.ensemble:
            E = self.sims.shape[1]
            sims = torch.as_tensor(self.sims, device=dev)
            worst_hist = torch.zeros((rows, A, R), **f64)
            mask_hist = torch.zeros((rows, A, R), dtype=torch.int64, device=dev)
            hists += [worst_hist, mask_hist]
            self.worst_max = np.empty((A, n_iter * R))
            self.refusing_members = np.empty((A, n_iter * R), dtype=np.int64)
            self.member_refusals = np.zeros((A, E), dtype=np.int64)
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
            got = [t.index_select(0, idx).cpu().numpy() for t in hists]
            tr = trace.index_select(0, idx).cpu().numpy() if costs == "all" else None
            for k, (it, _) in enumerate(pending):
                rets, cmax, ref, viol, stat = (g[k] for g in got[:5])
                if self.ensemble:
                    worst, mask = got[5][k], got[6][k]
                    self.worst_max[:, it * R:(it + 1) * R] = worst
                    self.refusing_members[:, it * R:(it + 1) * R] = mask
                    self.member_refusals += ((mask[:, :, None] >> np.arange(E)) & 1).sum(axis=1)
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
            if self.ensemble:
                safe_ars_rollouts_ensemble(self.params, H, policy, deltas, nu, gated, sims, sim_thr, real_thr,
                                           self.cost.kind, self.cost.index, returns=ret_hist[row], cost_trace=tr,
                                           cost_max=cmax_hist[row], first_refused=ref_hist[row],
                                           violations=viol_hist[row], status=stat_hist[row],
                                           worst_max=worst_hist[row], refusing_members=mask_hist[row])
            else:
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
