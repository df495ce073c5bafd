"""CACLA on the swimmer with safe exploration: the learner of cacla_agent.CACLA_agent inside the run loop of the
reference's safe agents (cacla/cacla_safe_agent.py:161-188, which the reference has for LQR only), every real step
gated by a one-step look-ahead in a simulator (safe_ars/ars.py:111-122) -- on the fused kernel behind
sw_cacla_safe_run_f64 (one wave per agent, whole chunks of steps in one launch).

The host side is CACLA_agent's: the initial weights from torch (actors first, then the critic), the exploration noise
from NumPy's legacy multivariate_normal, chunk by chunk.  The noise of a step is drawn whether or not the gate lets
the step through, so a plain and a safe agent started from the same seeds see the same weights and the same noise.

Rewards follow the reference's append rule (:177-188): nothing is appended before the first admitted step, and a
refused step repeats the last reward.  The kernel writes NaN where nothing is appended; trim_rewards() drops it.

The gate in an ENSEMBLE of simulators (sim_ensemble / sim_ensembles; ars/ensemble.py makes them): the look-ahead runs
in every member, up to 64 of them in the lanes of the agent's wave (sw_cacla_safe_ensemble_run_f64), and a step is
taken only where every member admits it.  The simulator threshold may then be None: the real threshold itself, the
worst member standing where the reference's unknown alpha * epsilon would.  Without an ensemble nothing changes: that
path is sw_cacla_safe_run_f64.
"""
import numpy as np
import torch

from . import safe_kernels
from .cacla_agent import chunk_sizes, draw_batch, draw_networks, run_chunks
from .._lib import STATUS_SINGULAR, dev_f64
from ..safe_ars.ars import NativeCost

CHUNK = 2048   # steps per launch, and per draw of the noise: CACLA_agent.chunk
MAX_MEMBERS = 64   # an agent's ensemble rides in the lanes of its wave (include/swimmer_hip.h)


def trim_rewards(rewards, admitted):
    """The reference's reward list from a run's rewards [n_iter] and admitted mask: the entries from the first
    admitted step on (before it the reference appends nothing); all of them absent when no step was admitted."""
    admitted = np.asarray(admitted, dtype=bool)
    hit = np.flatnonzero(admitted)
    return list(np.asarray(rewards)[hit[0]:]) if hit.size else []


def _native(cost):
    if not isinstance(cost, NativeCost) or cost.kind is None:
        raise TypeError("cost must be a safe_ars.NativeCost (AbsObs(i) / MaxAbsThetaDot()): the gate is evaluated "
                        f"in the kernel, not {type(cost).__name__}")
    return cost


def _same_model(env, sim_env):
    if (sim_env.n != env.n or sim_env.h != env.h
            or not np.array_equal(np.asarray(sim_env.direction, dtype=np.float64),
                                  np.asarray(env.direction, dtype=np.float64))):
        raise ValueError("sim_env must have the n, h and direction of env")


def _ensemble(members, what="sim_ensemble"):
    """A non-empty list of at most MAX_MEMBERS simulators."""
    members = list(members)
    if not members:
        raise ValueError(f"{what}: an ensemble needs at least one simulator")
    if len(members) > MAX_MEMBERS:
        raise ValueError(f"{what}: {len(members)} members; an ensemble has at most {MAX_MEMBERS}")
    return members


def member_rows(env, members, what="sim_ensemble"):
    """[E, 3] rows (l_i, m_i, k) of an ensemble's members -- objects with l_i, m_i, k, n, h (ars.EnvParam, SwimmerEnv)
    -- after checking each against env as _same_model does, the direction where the member has one."""
    for e, sp in enumerate(members):
        direction = getattr(sp, "direction", None)
        if (sp.n != env.n or sp.h != env.h
                or (direction is not None and not np.array_equal(np.asarray(direction, dtype=np.float64),
                                                                 np.asarray(env.direction, dtype=np.float64)))):
            raise ValueError(f"{what}[{e}] must have the n, h and direction of env")
    return np.array([[sp.l_i, sp.m_i, sp.k] for sp in members], dtype=np.float64)


class _SafeRun(object):
    """The device side of a run of A agents behind the gate: what cacla_agent._Run holds, plus the gate's inputs and
    the refusal bookkeeping.  draw(c) returns the next c steps' noise [A, c, m] on the host.  ensemble: sims is
    [A, E, 3], the run goes through the ensemble kernel and keeps worst_cost [A, n_iter] and member_refusals [A, E]."""

    def __init__(self, p, device, gammas, alphas, weights, state, gated, sims, sim_thresholds, real_thresholds, cost,
                 ensemble=False):
        self.p, self.device, self.cost = p, torch.device(device), cost
        self.ensemble, self.worst_cost = ensemble, None
        A = self.A = len(gammas)
        f64 = lambda v: dev_f64(np.asarray(v, dtype=np.float64), self.device)   # noqa: E731
        self.gamma, self.alpha = f64(gammas), f64(alphas)
        self.weights, self.state = dev_f64(weights, self.device), dev_f64(state, self.device)
        self.gated = torch.as_tensor(np.asarray(gated, dtype=np.int32), device=self.device)
        self.sim = f64(np.asarray(sims, dtype=np.float64).reshape((A, -1, 3) if ensemble else (A, 3)))
        self.member_refusals = (torch.zeros((A, self.sim.shape[1]), dtype=torch.int32, device=self.device)
                                if ensemble else None)
        self.sim_thresh, self.real_thresh = f64(sim_thresholds), f64(real_thresholds)
        self.last_reward = torch.full((A,), float("nan"), dtype=torch.float64, device=self.device)
        self.counters = torch.zeros((A, 3), dtype=torch.int32, device=self.device)
        self.first_refused = torch.full((A,), -1, dtype=torch.int32, device=self.device)
        self.status = torch.zeros(A, dtype=torch.int32, device=self.device)

    def run(self, n_iter, chunk, draw):
        """-> (rewards [A, n_iter], NaN before an agent's first admission; admitted bool [A, n_iter])."""
        sizes = chunk_sizes(n_iter, chunk)
        if not sizes:
            self.worst_cost = np.empty((self.A, 0)) if self.ensemble else None
            return np.empty((self.A, 0)), np.empty((self.A, 0), dtype=bool)

        kernel = safe_kernels.cacla_safe_ensemble_run if self.ensemble else safe_kernels.cacla_safe_run

        def launch(c, t, noise):   # -> the chunk's rewards and admit flags, and behind them an ensemble's worst costs
            rec = torch.empty((self.A, c), dtype=torch.int32, device=self.device)
            worst = torch.empty((self.A, c), dtype=torch.float64, device=self.device) if self.ensemble else None
            records = dict(worst_rec=worst, member_refusals=self.member_refusals) if self.ensemble else {}
            rewards = kernel(self.p, c, t, self.gamma, self.alpha, noise, self.gated, self.sim, self.sim_thresh,
                             self.real_thresh, self.cost.kind, self.cost.index, self.weights, self.state,
                             self.last_reward, self.counters, self.first_refused, admitted_rec=rec,
                             status=self.status, **records)
            return (rewards, rec, worst) if self.ensemble else (rewards, rec)

        rewards, admitted, *worst = run_chunks(self.device, self.A, self.p.m, sizes, draw, launch)
        self.worst_cost = worst[0] if self.ensemble else None
        return rewards, admitted.astype(bool)


class CACLA_SE_agent:
    """CACLA_agent behind a simulator gate; `env` and `sim_env` are swimmer_amd.SwimmerEnv objects with the same n, h
    and direction, `cost` a safe_ars.NativeCost.

    After run(): actor_weights [n - 1, net_doubles(n)], critic_weights [net_doubles(n)], initial_weights, admitted
    (steps taken), violations (steps taken whose cost exceeded real_threshold), actor_updates (steps with
    temp_diff > 0), first_refused (the first refused step, None if none), admitted_steps (bool [n_iter]) and status
    (SW_STATUS_* bits OR-ed over the run); the environment's state is the run's last.

    sim_ensemble: the gate in an ensemble of simulators instead of sim_env (which is then None) -- a non-empty list of
    at most 64 objects with l_i, m_i, k, n, h (ars.EnvParam, e.g. from ars.ensemble.sphere_ensemble /
    ensemble_from_estimates, or SwimmerEnv), each with env's n, h and -- where it has one -- direction; a step is
    taken only where every member admits it.  sim_threshold None is then the real threshold itself.  After run()
    there are also worst_cost [n_iter] (the largest member cost of each step, +inf for a NaN or a bad member) and
    member_refusals [E] (the steps each member's own cost refused: which member binds)."""

    chunk = CHUNK

    def __init__(self, gamma, alpha, sigma, sim_env, cost, real_threshold, sim_threshold, *, sim_ensemble=None):
        self.gamma, self.alpha, self.sigma = gamma, alpha, sigma
        if sim_ensemble is not None:
            if sim_env is not None:
                raise ValueError("give sim_env or sim_ensemble, not both")
            sim_ensemble = _ensemble(sim_ensemble)
            if sim_threshold is None:
                sim_threshold = real_threshold
        self.sim_env, self.sim_ensemble = sim_env, sim_ensemble
        self.cost = _native(cost)
        self.real_threshold, self.sim_threshold = real_threshold, sim_threshold
        self.worst_cost = self.member_refusals = None
        self.actor_weights = self.critic_weights = self.initial_weights = self.admitted_steps = None
        self.admitted = self.violations = self.actor_updates = self.status = 0
        self.first_refused = None

    def run(self, env, n_iter, H=1000):
        n, m = env.n, env.n - 1
        ensemble = self.sim_ensemble is not None
        if ensemble:
            sim = member_rows(env, self.sim_ensemble)                # [E, 3]
        else:
            _same_model(env, self.sim_env)
            sim = [self.sim_env.l_i, self.sim_env.m_i, self.sim_env.k]
        assert env.observation_space.shape[0] == 2 * n + 2 and env.action_space.shape[0] == m
        weights = draw_networks(n)                                   # torch's global generator
        self.initial_weights = weights.copy()
        state = np.asarray(env.reset(), dtype=np.float64)
        cov = self.sigma * np.identity(m)
        run = _SafeRun(env._params(), env.device, [self.gamma], [self.alpha], weights[None], state[None], [1], [sim],
                       [self.sim_threshold], [self.real_threshold], self.cost, ensemble=ensemble)
        rewards, admitted = run.run(int(n_iter), self.chunk,
                                    lambda c: np.random.multivariate_normal(np.zeros(m), cov, size=c)[None])
        rewards, self.admitted_steps = rewards[0], admitted[0]
        if ensemble:
            self.worst_cost = run.worst_cost[0]
            self.member_refusals = run.member_refusals.cpu().numpy()[0]
        w = run.weights.cpu().numpy()[0]
        self.actor_weights, self.critic_weights = w[:m].copy(), w[m].copy()
        self.status = int(run.status.cpu()[0])
        self.admitted, self.violations, self.actor_updates = (int(v) for v in run.counters.cpu().numpy()[0])
        first = int(run.first_refused.cpu()[0])
        self.first_refused = None if first < 0 else first
        if self.status & STATUS_SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")           # numpy.linalg.solve's, inside env.step
        env.set_state(run.state.cpu().numpy()[0].tolist())           # the environment has taken `admitted` steps
        for i in range(H, n_iter, H):
            if self.admitted_steps[:i + 1].any():                    # :190: only once there is a reward
                print(f"Iteration {i}/{n_iter}: reward: {rewards[i]}")
        return trim_rewards(rewards, self.admitted_steps)


class CACLA_SE_Batch(object):
    """A independent agents on one SwimmerEnv's model, gated or not, ONE launch per chunk of steps for all of them.

    Agent a has (gammas[a], alphas[a], sigmas[a]), the simulator sims[a] = (l_i, m_i, k) with the thresholds
    sim_thresholds[a] / real_thresholds[a], and draws its initial weights from torch.Generator().manual_seed(seeds[a])
    and its noise from np.random.RandomState(seeds[a]): row a is, bit for bit, the single
    agent after torch.manual_seed(seeds[a]); np.random.seed(seeds[a]) -- CACLA_SE_agent where gated[a] (default: all),
    CACLA_agent where not (its simulator and simulator threshold are not read; its violations are still counted).
    The global generators are not touched.

    run() returns (rewards [A, n_iter], NaN before an agent's first admission, and admitted bool [A, n_iter]).
    After it: weights [A, n, net_doubles(n)], state [A, d], status, admitted, violations, actor_updates and
    first_refused (-1: none) [A].

    sim_ensembles: the gate in an ensemble of simulators per agent instead of sims (which is then None) -- [A][E][3]
    rows (l_i, m_i, k), or a list of A lists of E members (objects as CACLA_SE_agent's sim_ensemble takes them), the
    same E <= 64 for every agent.  Row a is then the single CACLA_SE_agent(sim_ensemble=...) seeded seeds[a];
    sim_thresholds None is the real thresholds.  After run() there are also worst_cost [A, n_iter] (NaN in the rows of
    ungated agents) and member_refusals [A, E]."""

    def __init__(self, env, gammas, alphas, sigmas, seeds, sims, sim_thresholds, real_thresholds, cost, gated=None, *,
                 sim_ensembles=None):
        self.env, self.cost = env, _native(cost)
        self.seeds = [int(s) for s in seeds]
        A = self.n_agent = len(self.seeds)
        vec = lambda v: np.asarray(v, dtype=np.float64).reshape(-1)   # noqa: E731
        self.gammas, self.alphas, self.sigmas = vec(gammas), vec(alphas), vec(sigmas)
        self.ensemble = sim_ensembles is not None
        if self.ensemble:
            if sims is not None:
                raise ValueError("give sims or sim_ensembles, not both")
            if sim_thresholds is None:
                sim_thresholds = real_thresholds
            sims = self._ensemble_rows(env, sim_ensembles)            # [A, E, 3]
        self.sim_thresholds, self.real_thresholds = vec(sim_thresholds), vec(real_thresholds)
        self.sims = sims if self.ensemble else np.asarray(sims, dtype=np.float64).reshape(-1, 3)
        self.gated = np.ones(A, dtype=np.int32) if gated is None else (np.asarray(gated).reshape(-1) != 0).astype(np.int32)
        if A < 1 or not all(len(v) == A for v in (self.gammas, self.alphas, self.sigmas, self.sim_thresholds,
                                                  self.real_thresholds, self.sims, self.gated)):
            raise ValueError("gammas, alphas, sigmas, seeds, sims, the thresholds and gated must have the same "
                             "length, at least 1")
        self.weights = self.state = self.status = self.admitted = self.violations = self.actor_updates = None
        self.first_refused = self.worst_cost = self.member_refusals = None

    @staticmethod
    def _ensemble_rows(env, sim_ensembles):
        """[A, E, 3] from an array of rows or from A lists of members; every agent has the same number of them."""
        rows = []
        for a, members in enumerate(sim_ensembles):
            members = _ensemble(members, f"sim_ensembles[{a}]")
            rows.append(member_rows(env, members, f"sim_ensembles[{a}]") if hasattr(members[0], "l_i")
                        else np.asarray(members, dtype=np.float64))
        if any(r.ndim != 2 or r.shape[1] != 3 for r in rows) or len({r.shape[0] for r in rows}) > 1:
            raise ValueError("sim_ensembles: every agent needs the same number of members, rows (l_i, m_i, k); "
                             "per-agent ensemble sizes are not built")
        return np.stack(rows) if rows else np.empty((0, 1, 3))

    def run(self, n_iter, chunk=2048):
        env = self.env
        weights, draw, state = draw_batch(env, self.seeds, self.sigmas)
        run = _SafeRun(env._params(), env.device, self.gammas, self.alphas, weights, state, self.gated, self.sims,
                       self.sim_thresholds, self.real_thresholds, self.cost, ensemble=self.ensemble)
        rewards, admitted = run.run(int(n_iter), int(chunk), draw)
        if self.ensemble:
            self.worst_cost = run.worst_cost
            self.member_refusals = run.member_refusals.cpu().numpy()
        self.weights = run.weights.cpu().numpy()
        self.state = run.state.cpu().numpy()
        self.status = run.status.cpu().numpy()
        counters = run.counters.cpu().numpy()
        self.admitted, self.violations, self.actor_updates = counters[:, 0], counters[:, 1], counters[:, 2]
        self.first_refused = run.first_refused.cpu().numpy()
        return rewards, admitted
