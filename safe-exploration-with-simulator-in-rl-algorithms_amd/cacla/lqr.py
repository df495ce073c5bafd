"""CACLA on LQR problems, with and without safe exploration, on the fused kernel (kernels.lqr_cacla_run): the host
side shared by CACLA_LQR_agent (cacla_agent.py), the four safe agents (cacla_safe_agent.py) and CACLA_LQR_Batch.

The whole learner -- linear actor, Gaussian action, the simulator's step and the gate on its cost, the real step,
temporal difference, critic update, conditional actor update -- runs on the GPU for whole chunks of steps, one agent
per lane.  What stays on the host is what fixes the random streams, drawn exactly as the reference draws them: the
initial state `rand(ns)` of env.reset(), then per chunk `multivariate_normal(zeros, sigma I, size=c)`, which consumes
the stream as c of the reference's per-step `multivariate_normal(FA_act, sigma I)` do and returns their noise (the
mean is added last there, and in the kernel).  The draws do not depend on whether a step is admitted.  `sigma` is the
VARIANCE of the policy, as in the reference.

Costs.  The kernel knows three costs of a state: its inf-, 2- and 1-norm.  norm_cost(ord) is such a cost as a small
callable that also works on the host; a plain callable (the reference's `lambda x: np.linalg.norm(x, np.inf)`) is
accepted when it agrees EXACTLY with one of the three on COST_PROBES (cost_code); anything else is a TypeError.
"""
import numpy as np
import torch

from .. import kernels
from .._lib import STATUS_NONFINITE, SwimmerHipError, dev_f64  # noqa: F401
from ..envs.gym_lqr.lqr_env import model_of
from .cacla_agent import Uploader

CHUNK = 2048      # steps per launch
KINDS = ("plain", "se", "fix", "bounded", "affine")
RECORDS = ("states", "actions", "rewards", "admitted")

# The probe set of cost_code(): a callable is taken for a norm when it returns exactly that norm on the first ns
# columns of every row (signs, a zero, ties between coordinates and magnitudes from 1e-4 to 7 are all in it).
COST_PROBES = np.array([[3.0, -4.0, 1.0, -2.0],
                        [-0.5, 0.25, -2.0, 1.5],
                        [1.0, 1.0, 1.0, 1.0],
                        [0.0, -7.0, 0.0, 0.0],
                        [-1.25, 2.5, -3.75, 0.5],
                        [1e-3, -2e-3, 5e-4, -1e-4]])
_ORDS = ((np.inf, kernels.LQR_COST_INF), (2, kernels.LQR_COST_2), (1, kernels.LQR_COST_1))


class norm_cost(object):
    """cost(state) = numpy.linalg.norm(state, ord), ord one of np.inf, 2, 1: a cost the kernel evaluates itself."""

    def __init__(self, ord=np.inf):
        if not any(ord == o for o, _ in _ORDS):
            raise TypeError("norm_cost: ord must be np.inf, 2 or 1")
        self.ord = ord

    def __call__(self, state):
        return np.linalg.norm(np.asarray(state, dtype=np.float64), self.ord)

    def __repr__(self):
        return f"norm_cost({self.ord})"


def cost_code(cost, ns):
    """The kernel's code (kernels.LQR_COST_*) of a Constraint's cost for states of dimension ns."""
    if isinstance(cost, norm_cost):
        return dict(_ORDS)[cost.ord]
    if callable(cost):
        probes = COST_PROBES[:, :ns]
        try:
            got = [cost(x.copy()) for x in probes]
            for ord_, code in _ORDS:          # ns = 1: the three coincide, and the first is as good as any
                if all(np.ndim(g) == 0 and g == np.linalg.norm(x, ord_) for g, x in zip(got, probes)):
                    return code
        except Exception:                      # noqa: BLE001 -- a callable that cannot take a state is not a cost
            pass
    raise TypeError("Constraint.cost must be norm_cost(np.inf), norm_cost(2) or norm_cost(1), or a callable equal to "
                    "numpy.linalg.norm(x, np.inf | 2 | 1): the kernel evaluates the inf-, 2- and 1-norm of the state "
                    f"only (got {cost!r})")


def pack_params(real, sim, gamma, alpha, l=0.0, eps_lc=0.0, dA=0.0, dB=0.0, threshold=0.0):
    """One agent's column of the kernel's parameter block (include/swimmer_hip.h, SW_LQR_PARAM_DOUBLES): real and sim
    are model_of() tuples (sim None: the real model again; a plain run does not read it)."""
    A, B, C, max_s, max_a, Q, R = real
    sA, sB, sC, s_max_s, s_max_a = (real if sim is None else sim)[:5]
    if sA.shape != A.shape or sB.shape != B.shape:
        raise ValueError("the simulator must have the real environment's dimensions")
    return np.concatenate([A.reshape(-1), B.reshape(-1), C, [max_s, max_a], sA.reshape(-1), sB.reshape(-1), sC,
                           [s_max_s, s_max_a], Q.reshape(-1), R.reshape(-1),
                           [gamma, alpha, l, eps_lc, dA, dB, threshold]]).astype(np.float64)


def fixed_threshold(kind, real_env, sim_env, epsilon, constraint, L_theta=None):
    """The simulator threshold of the fixed-threshold agents, in the reference's order of operations:
    l - epsilon * L_c * L_theta with L_theta given ("fix": set_simulator_threshold), from the bounds ("bounded",
    cacla_safe_agent.py:215) or the affine problem's constant ("affine", :227)."""
    if kind == "bounded":
        n_obs = real_env.observation_space.shape[0]
        n_ac = real_env.action_space.shape[0]
        L_theta = (sim_env.op_norm_der_A * np.sqrt(n_obs) * real_env.max_s
                   + sim_env.op_norm_der_B * np.sqrt(n_ac) * real_env.max_a)
    elif kind == "affine":
        L_theta = np.linalg.norm(np.array([0.1, 0]))
    elif L_theta is None:
        raise ValueError("a fixed-threshold agent needs its L_theta (set_simulator_threshold)")
    return constraint.l - epsilon * constraint.L_c * L_theta


def agent_column(kind, real_env, gamma, alpha, sim_env=None, epsilon=None, constraint=None, threshold=None):
    """(column of the parameter block, cost code) of one agent of `kind`; threshold: the fixed kinds' simulator
    threshold (fixed_threshold())."""
    real = model_of(real_env)
    if kind == "plain":
        return pack_params(real, None, gamma, alpha), kernels.LQR_COST_INF
    if sim_env is None or epsilon is None or constraint is None:
        raise ValueError(f"a {kind!r} agent needs a simulator, epsilon and a constraint")
    code = cost_code(constraint.cost, real[0].shape[0])
    return pack_params(real, model_of(sim_env), gamma, alpha, constraint.l, epsilon * constraint.L_c,
                       getattr(sim_env, "op_norm_der_A", 0.0), getattr(sim_env, "op_norm_der_B", 0.0),
                       0.0 if threshold is None else threshold), code


class Run(object):
    """The device side of a run of A agents of one kind and shape: parameter block, F, V, state, the last admitted
    record, counters, status, and the chunk loop.  Everything is agent-minor on the device and agent-major here."""

    def __init__(self, kind, ns, na, cost, params, F, V, state, device="cuda:0"):
        if kind not in KINDS:
            raise ValueError(f"agent must be one of {KINDS}, not {kind!r}")
        if not (1 <= ns <= kernels.LQR_MAX_STATE and 1 <= na <= kernels.LQR_MAX_ACTION):
            raise SwimmerHipError(f"the LQR kernel takes 1..{kernels.LQR_MAX_STATE} state and 1.."
                                  f"{kernels.LQR_MAX_ACTION} action dimensions, not ({ns}, {na})")
        self.kind, self.ns, self.na, self.cost = kind, ns, na, int(cost)
        self.safe = kind != "plain"
        self.threshold = kernels.LQR_THRESHOLD_STEP if kind in ("plain", "se") else kernels.LQR_THRESHOLD_FIXED
        self.device = torch.device(device)
        params = np.asarray(params, dtype=np.float64)
        A = self.A = params.shape[0]
        self.params = dev_f64(params.T, self.device)
        self.F = dev_f64(np.asarray(F, dtype=np.float64).reshape(A, na * ns).T.reshape(na, ns, A), self.device)
        self.V = dev_f64(np.asarray(V, dtype=np.float64).reshape(A, ns).T, self.device)
        self.state = dev_f64(np.asarray(state, dtype=np.float64).reshape(A, ns).T, self.device)
        self.last = torch.zeros((ns + na + 1, A), dtype=torch.float64, device=self.device)
        self.counters = torch.zeros((3, A), dtype=torch.int32, device=self.device)
        self.status = torch.zeros(A, dtype=torch.int32, device=self.device)

    def run(self, n_iter, chunk, draw, record=RECORDS):
        """draw(c) -> the next c steps' noise [A, c, na] on the host.  Returns {name: host array} for the names in
        `record`: states [A, n_iter, ns], actions [A, n_iter, na], rewards [A, n_iter], admitted uint8 [A, n_iter]."""
        ns, na, A = self.ns, self.na, self.A
        unknown = [r for r in record if r not in RECORDS]
        if unknown:
            raise ValueError(f"record: unknown {unknown}; choose from {RECORDS}")
        if n_iter < 0 or chunk < 1:
            raise SwimmerHipError("n_iter must be >= 0 and chunk >= 1")
        shapes = {"states": (ns, A), "actions": (na, A), "rewards": (A,), "admitted": (A,)}
        kept = {r: [] for r in record}
        sizes = [min(chunk, n_iter - t) for t in range(0, n_iter, chunk)]
        with torch.cuda.device(self.device):
            up = Uploader(max(sizes, default=0) * na * A, self.device) if sizes else None
            for c in sizes:
                noise = up.upload(np.ascontiguousarray(np.transpose(draw(c), (1, 2, 0))))
                rec = {r: torch.empty((c,) + shapes[r], dtype=torch.uint8 if r == "admitted" else torch.float64,
                                      device=self.device) for r in record}
                kernels.lqr_cacla_run(ns, na, c, self.safe, self.threshold, self.cost, self.params, noise, self.F,
                                      self.V, self.state, self.last, self.counters, self.status,
                                      rec_state=rec.get("states"), rec_action=rec.get("actions"),
                                      rec_reward=rec.get("rewards"), rec_admitted=rec.get("admitted"))
                for r in record:
                    kept[r].append(rec[r])
            out = {}
            for r in record:
                dt = np.uint8 if r == "admitted" else np.float64
                full = (torch.cat(kept[r]).cpu().numpy() if kept[r] else np.empty((0,) + shapes[r], dtype=dt))
                out[r] = np.ascontiguousarray(np.moveaxis(full, -1, 0))      # [T, .., A] -> [A, T, ..]
        return out

    def finals(self):
        """(F [A, na, ns], V [A, ns], state [A, ns], admitted, violations, actor_updates, status [A]) on the host."""
        A = self.A
        F = np.ascontiguousarray(self.F.cpu().numpy().reshape(self.na * self.ns, A).T).reshape(A, self.na, self.ns)
        V = np.ascontiguousarray(self.V.cpu().numpy().T)
        state = np.ascontiguousarray(self.state.cpu().numpy().T)
        counters = self.counters.cpu().numpy()
        return F, V, state, counters[0].copy(), counters[1].copy(), counters[2].copy(), self.status.cpu().numpy()


def reference_arrays(states, actions, rewards, admitted):
    """One agent's records [n_iter, ..] as the reference returns them: its lists repeat the last entry at a refused
    step (the kernel's records do too) and get NOTHING at a refused step before the first admitted one, so the arrays
    start at the first admitted step -- np.array([]) each when there is none."""
    first = np.flatnonzero(admitted != kernels.LQR_NOTHING_YET)
    if first.size == 0:
        return np.array([]), np.array([]), np.array([])
    f = first[0]
    return states[f:], actions[f:], rewards[f:]


def run_single(agent, kind, n_iter, gamma, alpha, sigma, H, sim_env=None, epsilon=None, constraint=None,
               threshold=None):
    """The body of every single agent's run(): the reference's loop on the global NumPy stream."""
    env = agent.env
    ns, na = agent.F.shape[1], agent.F.shape[0]
    n_iter = int(n_iter)
    column, cost = agent_column(kind, env, gamma, alpha, sim_env, epsilon, constraint, threshold)
    state = np.asarray(env.reset(), dtype=np.float64)
    cov = sigma * np.identity(na)
    zeros = np.zeros(na)
    run = Run(kind, ns, na, cost, column[None], agent.F[None], agent.V[None], state[None],
              getattr(agent, "device", "cuda:0"))
    rec = run.run(n_iter, agent.chunk, lambda c: np.random.multivariate_normal(zeros, cov, size=c)[None])
    F, V, final, admitted, violations, actor_updates, status = run.finals()
    agent.F, agent.V = F[0], V[0]
    agent.admitted, agent.violations = int(admitted[0]), int(violations[0])
    agent.actor_updates, agent.status = int(actor_updates[0]), int(status[0])
    env.set_state(final[0])                                # the environment has taken the admitted steps
    states, actions, rewards = reference_arrays(rec["states"][0], rec["actions"][0], rec["rewards"][0],
                                                rec["admitted"][0])
    skipped = n_iter - len(rewards)                        # refused steps before the first admitted one
    for i in range(H, n_iter, H) if H > 0 else ():
        if i >= skipped:                                   # the reference would raise NameError before (or prints nothing)
            print(f"Iteration {i}/{n_iter}: reward: {rewards[i - skipped]}")
    return states, actions, rewards


class CACLA_LQR_Batch(object):
    """A independent CACLA agents on LQR problems, ONE launch per chunk of steps for all of them.

    real_envs: one environment per agent, or one for all; sim_envs likewise (safe kinds); gammas, alphas, sigmas,
    epsilons: one value per agent or one for all; constraints: one Constraint per agent or one for all (all with the
    same cost); agent: "plain" (CACLA_LQR_agent), "se" (CACLA_LQR_SE_agent), "fix" (CACLA_LQR_SE_fix, with L_thetas =
    what each would be given to set_simulator_threshold), "bounded" or "affine".  All agents share the dimensions.

    Agent a draws its initial state and its noise from np.random.RandomState(seeds[a]) and starts from F = V = 0:
    row a is, bit for bit, what the single agent's run() gives after np.random.seed(seeds[a]).  The global stream and
    the environments are not touched.

    run(n_iter, chunk=2048, record=("states", "actions", "rewards", "admitted")) returns {name: array} of the chosen
    per-step records, full length ([A, n_iter, ..]; `admitted` holds kernels.LQR_ADMITTED / LQR_REFUSED /
    LQR_NOTHING_YET); arrays_of(a) cuts agent a's down to what the reference returns.  record=() keeps nothing: a
    long run of a large batch needs no memory per step.  After run(): F [A, na, ns], V [A, ns], state [A, ns],
    admitted, violations, actor_updates, status [A]."""

    def __init__(self, real_envs, gammas, alphas, sigmas, seeds, sim_envs=None, epsilons=None, constraints=None,
                 agent="plain", L_thetas=None, device="cuda:0"):
        if agent not in KINDS:
            raise ValueError(f"agent must be one of {KINDS}, not {agent!r}")
        self.seeds = [int(s) for s in seeds]
        A = self.n_agent = len(self.seeds)
        if A < 1:
            raise ValueError("at least one seed")

        def each(v, name):
            if v is None:
                return [None] * A
            v = list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * A
            if len(v) != A:
                raise ValueError(f"{name}: one per agent ({A}) or one for all, got {len(v)}")
            return v
        self.kind, self.device = agent, device
        self.real_envs, self.sim_envs = each(real_envs, "real_envs"), each(sim_envs, "sim_envs")
        self.gammas, self.alphas, self.sigmas = each(gammas, "gammas"), each(alphas, "alphas"), each(sigmas, "sigmas")
        self.epsilons, self.constraints = each(epsilons, "epsilons"), each(constraints, "constraints")
        self.L_thetas = each(L_thetas, "L_thetas")
        columns, codes = [], set()
        for a in range(A):
            thr = None
            if agent in ("fix", "bounded", "affine"):
                if self.sim_envs[a] is None or self.epsilons[a] is None or self.constraints[a] is None:
                    raise ValueError(f"a {agent!r} agent needs a simulator, epsilon and a constraint")
                thr = fixed_threshold(agent, self.real_envs[a], self.sim_envs[a], self.epsilons[a],
                                      self.constraints[a], self.L_thetas[a])
            col, code = agent_column(agent, self.real_envs[a], self.gammas[a], self.alphas[a], self.sim_envs[a],
                                     self.epsilons[a], self.constraints[a], thr)
            columns.append(col)
            codes.add(code)
        if len({len(c) for c in columns}) != 1:
            raise ValueError("all agents of a batch must have the same state and action dimensions")
        if len(codes) != 1:
            raise ValueError("all constraints of a batch must have the same cost")
        self.cost = codes.pop()
        self.params = np.stack(columns)
        self.ns = np.asarray(self.real_envs[0].A).shape[1]
        self.na = np.asarray(self.real_envs[0].B).shape[1]
        self.F = self.V = self.state = self.admitted = self.violations = self.actor_updates = self.status = None
        self.records = {}

    def run(self, n_iter, chunk=CHUNK, record=RECORDS):
        A, ns, na = self.n_agent, self.ns, self.na
        streams = [np.random.RandomState(s) for s in self.seeds]
        state = np.stack([rs.rand(ns) for rs in streams])                    # env.reset()
        covs = [s * np.identity(na) for s in self.sigmas]
        zeros = np.zeros(na)

        def draw(c):
            return np.stack([rs.multivariate_normal(zeros, cov, size=c) for rs, cov in zip(streams, covs)])

        run = Run(self.kind, ns, na, self.cost, self.params, np.zeros((A, na, ns)), np.zeros((A, ns)), state,
                  self.device)
        self.records = run.run(int(n_iter), int(chunk), draw, tuple(record))
        (self.F, self.V, self.state, self.admitted, self.violations, self.actor_updates, self.status) = run.finals()
        return self.records

    def arrays_of(self, a):
        """(states, actions, rewards) of agent a as its single agent's run() returns them (needs all four records)."""
        r = self.records
        return reference_arrays(r["states"][a], r["actions"][a], r["rewards"][a], r["admitted"][a])
