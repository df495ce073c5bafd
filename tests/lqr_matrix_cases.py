"""Generated cases for every compiled instantiation of the LQR kernel (lqr_cacla_kernel<NS, NA, MODE>, ns 1..4 x na
1..2 x plain / step threshold / fixed threshold) and every cost code: 67 agents (one full wave and three lanes) of 100
steps (no multiple of the kernel's noise block), every agent with its own models, Q, R, hyper-parameters, F0, V0,
initial state and noise.  case() gives the kernel's inputs, oracle() what tests/lqr_oracle.py makes of them.

The inputs of a shape and cost do not depend on the mode: the step-threshold run, the fixed-threshold run and (at the
inf-norm) the plain run of a shape start from the same agents.  tests/test_lqr_matrix_cpu.py checks, on the oracle
alone, that these inputs exercise what the GPU comparison (tests/test_lqr_matrix_gpu.py) is meant to catch; SEEDS and
the constants below were chosen until all of its conditions held for every agent of every case.
"""
import functools

import numpy as np

from swimmer_amd import kernels
from swimmer_amd.cacla import lqr

import lqr_oracle

AGENTS, STEPS = 67, 100
SHAPES = tuple((ns, na) for ns in range(1, kernels.LQR_MAX_STATE + 1) for na in range(1, kernels.LQR_MAX_ACTION + 1))
PLAIN, STEP, FIXED = 0, 1, 2                                   # the kernel's MODE
KINDS = {PLAIN: "plain", STEP: "se", FIXED: "fix"}             # lqr.Run's kind of a mode
COSTS = (kernels.LQR_COST_INF, kernels.LQR_COST_2, kernels.LQR_COST_1)
ORDS = {kernels.LQR_COST_INF: np.inf, kernels.LQR_COST_2: 2, kernels.LQR_COST_1: 1}
# the seven launches of a shape: (mode, cost)
VARIANTS = ((PLAIN, kernels.LQR_COST_INF),) + tuple((m, c) for m in (STEP, FIXED) for c in COSTS)

BOUNDS = ("none", "both", "action")                            # cycled over the agents
ALPHAS = (3e-3, 1e-3, 3e-4, 2e-3, 5e-4)
GAMMAS = (1.0, 0.9, 0.5, 0.95)
NOISE_STD = (0.4, 0.2, 0.1)
SIM_ERROR = (0.03, 0.06, 0.1)                                  # relative error of the simulator's A and B
FIXED_MARGIN = (0.1, 0.02, 0.05, 0.0)                          # fixed threshold = l - margin
MAX_A_NORM = 1.4                                               # largest singular value of A
MAX_S_QUANTILE = (0.7, 0.95)                                   # max_s = that quantile of an unbounded run's max |s_j|
L_QUANTILE, L_MARGIN = (0.8, 1.0), (0.05, 0.2)                 # l = that quantile of a plain run's costs + margin
START, LATE_START = (0.3, 0.9), (1.3, 2.0)                     # cost of the initial state, in units of l
MAX_CLOSED_LOOP_RADIUS = 0.97                                  # of A + B F0: no agent diverges in 100 steps

# seed of a (ns, na, cost) where the default, 1000 ns + 100 na + cost, leaves a condition of the CPU test unmet
SEEDS = {(1, 2, kernels.LQR_COST_INF): 1220}


def seed_of(ns, na, cost):
    """At ns = 1 the three costs are one function and share their agents: their launches must agree bit for bit."""
    cost = kernels.LQR_COST_INF if ns == 1 else cost
    return SEEDS.get((ns, na, cost), 1000 * ns + 100 * na + cost)


def _radius(M):
    return float(np.abs(np.linalg.eigvals(M)).max())


def _costs(m, F, x0, noise, ord_):
    """The cost of every state of the run of model m under the fixed actor F: no gate, no learning."""
    s, out = x0, []
    for u in noise:
        s, _ = lqr_oracle.env_step(m, s, F @ s + u)
        out.append(np.linalg.norm(s, ord_))
    return out


def _agent(rs, ns, na, k, ord_):
    """Agent k's inputs: dict(real, sim: lqr_oracle.model() tuples; Q, R, gamma, alpha, l, eps_lc, dA, dB, thr_fixed,
    F0, V0, x0, noise)."""
    while True:                                                # no strong transient growth: rewards stay small
        A = rs.uniform(-1, 1, (ns, ns))
        A *= rs.uniform(0.5, 0.95) / _radius(A)
        if np.linalg.norm(A, 2) <= MAX_A_NORM:
            break
    B = rs.uniform(0.3, 0.8, (ns, na)) * rs.choice([-1.0, 1.0], (ns, na))
    C = rs.uniform(-0.2, 0.2, ns) if k % 2 else np.zeros(ns)
    bound = BOUNDS[k % 3]
    max_a = 0.0 if bound == "none" else rs.uniform(0.3, 0.7)
    F0 = rs.uniform(-0.3, 0.3, (na, ns))
    while _radius(A + B @ F0) > MAX_CLOSED_LOOP_RADIUS:
        F0 *= 0.5
    x0 = rs.rand(ns)
    noise = rs.normal(0.0, NOISE_STD[(k + k // 3) % 3], (STEPS, na))
    # max_s: a quantile of the largest coordinate along the agent's own ungated, unlearning run, so that clip_s acts
    max_s = 0.0
    if bound == "both":
        max_s = float(np.quantile(_costs((A, B, C, 0.0, max_a), F0, x0, noise, np.inf), rs.uniform(*MAX_S_QUANTILE)))
    err = SIM_ERROR[(k // 3) % 3]
    # the simulator's bounds differ from the real ones too: a kernel that clips its step at the real bounds shows
    sim = (A * (1 + err * rs.uniform(-1, 1, A.shape)), B * (1 + err * rs.uniform(-1, 1, B.shape)), C * 0.9,
           max_s * 0.97, max_a * 1.04)
    M = rs.uniform(-1, 1, (ns, ns))
    Q = M @ M.T / (2 * ns) + 0.5 * np.eye(ns)
    M = rs.uniform(-1, 1, (na, na))
    R = M @ M.T / na + 0.5 * np.eye(na)
    # l: a quantile of the cost along that run with the bounds in place, so that the gate has work to do
    l = float(np.quantile(_costs((A, B, C, max_s, max_a), F0, x0, noise, ord_), rs.uniform(*L_QUANTILE)))
    l += rs.uniform(*L_MARGIN)
    # the run starts inside the limit, or (every 8th agent) well outside it: refused until the noise lets it in
    x0 = x0 / np.linalg.norm(x0, ord_) * l * (rs.uniform(*LATE_START) if k % 8 == 3 else rs.uniform(*START))
    return dict(real=(A, B, C, max_s, max_a), sim=sim, Q=Q, R=R, gamma=GAMMAS[k % 4], alpha=ALPHAS[k % 5], l=l,
                eps_lc=rs.uniform(0.02, 0.1), dA=rs.uniform(0.1, 1.0), dB=rs.uniform(0.1, 1.0),
                thr_fixed=l - FIXED_MARGIN[k % 4], F0=F0, V0=-rs.uniform(1, 4, ns), x0=x0,
                noise=noise)


@functools.lru_cache(maxsize=None)
def agents(ns, na, cost):
    """The 67 agents of a shape and cost (the same for every mode)."""
    rs = np.random.RandomState(seed_of(ns, na, cost))
    return tuple(_agent(rs, ns, na, k, ORDS[cost]) for k in range(AGENTS))


def case(ns, na, mode, cost):
    """The kernel's inputs of one launch: dict(kind, columns [A, SW_LQR_PARAM_DOUBLES], F0 [A, na, ns], V0 [A, ns],
    x0 [A, ns], noise [A, T, na], agents: the per-agent inputs).  A plain run's simulator block is the real model."""
    if mode == PLAIN and cost != kernels.LQR_COST_INF:
        raise ValueError("a plain run has no cost: its case is the inf-norm's agents")
    ag = agents(ns, na, cost)
    columns = [lqr.pack_params(a["real"] + (a["Q"], a["R"]), None if mode == PLAIN else a["sim"], a["gamma"],
                               a["alpha"], a["l"], a["eps_lc"], a["dA"], a["dB"], a["thr_fixed"]) for a in ag]
    return dict(kind=KINDS[mode], columns=np.stack(columns), F0=np.stack([a["F0"] for a in ag]),
                V0=np.stack([a["V0"] for a in ag]), x0=np.stack([a["x0"] for a in ag]),
                noise=np.stack([a["noise"] for a in ag]), agents=ag)


@functools.lru_cache(maxsize=None)
def oracle(ns, na, mode, cost, ord_=None, sim_is_real=False):
    """lqr_oracle.run on every agent of case(ns, na, mode, cost): a tuple of its dicts.  ord_: the norm to gate on in
    place of the case's; sim_is_real: the real model in the simulator's place.  (Computed once per process.)"""
    out = []
    for a in agents(ns, na, cost):
        safe = {}
        if mode != PLAIN:
            safe = dict(sim=a["real"] if sim_is_real else a["sim"], threshold="step" if mode == STEP else "fixed",
                        ord=ORDS[cost] if ord_ is None else ord_, l=a["l"], eps_lc=a["eps_lc"], dA=a["dA"], dB=a["dB"],
                        thr_fixed=a["thr_fixed"])
        out.append(lqr_oracle.run(a["real"], a["Q"], a["R"], a["gamma"], a["alpha"], a["x0"], a["noise"], F0=a["F0"],
                                  V0=a["V0"], **safe))
    return tuple(out)
