"""Plain NumPy restatement of ONE CACLA agent on an LQR problem, plain or with safe exploration (the reference's
cacla/cacla_agent.py:202-297, cacla/cacla_safe_agent.py, envs/gym_lqr/lqr_env.py), for the tests: the initial state
and the noise are INPUTS.  It is the step written out in include/swimmer_hip.h (sw_lqr_cacla_run_f64), and what the
kernel is compared with where there is no golden.

Also the table of the golden cases (CASES) and how a case's environments, constraint and agent are built from a set
of classes -- the reference's (tests/golden/make_lqr_golden.py) or this package's (the tests): build().
"""
import numpy as np

# tag: agent kind, environment, seed, (theta_real, theta_sim), steps, gamma, alpha, sigma, l; `extra`: the bounds
# (max_s, max_a) or (max_a,); epsilon: |theta_real - theta_sim| unless given.  Cost: the inf-norm, L_c = 1.
CASES = {
    "S1": dict(kind="se", env="easy", seed=0, theta=(1.0, 0.99), steps=512, gamma=1, alpha=1e-4, sigma=0.1, l=4),
    "S2": dict(kind="se", env="easy", seed=4, theta=(0.9, 0.85), steps=512, gamma=0.9, alpha=1e-2, sigma=1.0, l=1.5),
    "S4": dict(kind="bounded", env="bounded", extra=(1.0, 0.5), seed=5, theta=(0.95, 0.9), steps=512, gamma=0.9,
               alpha=1e-2, sigma=1.0, l=1.0),
    "S5": dict(kind="bounded", env="bounded", extra=(2.0, 1.0), seed=6, theta=(0.95, 0.9), steps=512, gamma=0.9,
               alpha=1e-2, sigma=1.0, l=1.5),
    "S6": dict(kind="bounded", env="bounded_action", extra=(1.0,), seed=7, theta=(0.95, 0.9), steps=512, gamma=0.9,
               alpha=1e-2, sigma=1.0, l=1.5),
    "S7": dict(kind="affine", env="affine", seed=9, theta=(1.0, 0.99), steps=512, gamma=1, alpha=1e-4, sigma=0.1, l=4),
    "S8": dict(kind="bounded", env="bounded", extra=(2.0, 1.0), seed=0, theta=(0.9, 0.8), steps=512, gamma=0.9,
               alpha=1e-3, sigma=0.1, l=0.8),
    "L32": dict(kind="se", env="easy", seed=32, theta=(0.9, 0.85), steps=256, gamma=0.9, alpha=1e-2, sigma=0.1, l=0.5),
    "V0": dict(kind="se", env="easy", seed=0, theta=(1.0, 0.8), epsilon=0, steps=256, gamma=0.9, alpha=1e-2,
               sigma=1.0, l=1.0),
    "P11": dict(kind="plain", env="ones", seed=11, steps=1000, gamma=1, alpha=1e-3, sigma=0.1),
    "P12": dict(kind="plain", env="lqr2", seed=12, steps=1000, gamma=1, alpha=1e-2, sigma=0.1),
    "P13": dict(kind="plain", env="p13", seed=13, steps=1000, gamma=0.9, alpha=1e-2, sigma=0.3),
}
P13 = dict(A=np.array([[.5, .2, 0], [0, .6, .3], [.1, 0, .7]]), B=np.array([[1., 0], [0, 1], [.5, .5]]),
           Q=np.array([[2, .5, 0], [.5, 1, 0], [0, 0, 1]]), R=np.array([[1, .2], [.2, .5]]))
ENV_CLASSES = ("LinearQuadReg", "EasyParamLinearQuadReg", "BoundedEasyLinearQuadReg",
               "BoundedActionEasyLinearQuadReg", "EasyAffineQuadReg")


def make_env(envs, name, theta=None, extra=()):
    """One environment of a case from the classes in `envs` (a module with the reference's class names)."""
    if name == "ones":
        return envs.LinearQuadReg(np.ones((1, 1)), np.ones((1, 1)), np.ones((1, 1)), np.ones((1, 1)))
    if name == "lqr2":
        return envs.LinearQuadReg(np.array([[0, 1], [1, 0]]), np.array([[0], [1]]), np.array([[1, 0], [0, 1]]),
                                  np.array([[1]]))
    if name == "p13":
        return envs.LinearQuadReg(P13["A"].copy(), P13["B"].copy(), P13["Q"].copy(), P13["R"].copy())
    cls = {"easy": envs.EasyParamLinearQuadReg, "bounded": envs.BoundedEasyLinearQuadReg,
           "bounded_action": envs.BoundedActionEasyLinearQuadReg, "affine": envs.EasyAffineQuadReg}[name]
    return cls(theta, *extra)


def epsilon_of(case):
    return case.get("epsilon", abs(case["theta"][0] - case["theta"][1])) if "theta" in case else None


def build(case, envs, plain_cls, safe, constraint_cls=None):
    """-> (agent, real_env, sim_env) of a case: envs, plain_cls (CACLA_LQR_agent) and safe (the module with Constraint
    and the safe agents) are the reference's or this package's.  The cost is the reference script's lambda."""
    if case["kind"] == "plain":
        real = make_env(envs, case["env"])
        return plain_cls(real), real, None
    extra = case.get("extra", ())
    real = make_env(envs, case["env"], case["theta"][0], extra)
    sim = make_env(envs, case["env"], case["theta"][1], extra)
    constraint = (constraint_cls or safe.Constraint)(lambda x: np.linalg.norm(x, np.inf), case["l"], 1)
    cls = {"se": safe.CACLA_LQR_SE_agent, "bounded": safe.CACLA_Bounded_LQR_SE_agent,
           "affine": safe.CACLA_AffineQR_SE_agent}[case["kind"]]
    return cls(real, sim, epsilon_of(case), constraint), real, sim


def clip(x, M):
    """reset_inbound as coded: M == 0 no bound, else |x_i| > M -> |x_i| / x_i * M.  A copy."""
    x = np.array(x, dtype=np.float64)
    if M != 0:
        big = np.abs(x) > M
        if big.any():
            with np.errstate(invalid="ignore", divide="ignore"):
                x[big] = np.abs(x[big]) / x[big] * M
    return x


def model(env):
    """(A, B, C, max_s, max_a) of an environment object as float64."""
    A, B = np.asarray(env.A, dtype=np.float64), np.asarray(env.B, dtype=np.float64)
    C = np.asarray(getattr(env, "C", np.zeros(A.shape[0])), dtype=np.float64)
    return A, B, C, float(getattr(env, "max_s", 0)), float(getattr(env, "max_a", 0))


def env_step(m, s, u):
    return step_counted(m, s, u)[:2]


def step_counted(m, s, u):
    """env_step and whether (clip_a changed the action, clip_s changed the state)."""
    A, B, C, max_s, max_a = m
    a = clip(u, max_a)
    raw = A @ s + B @ a + C
    sn = clip(raw, max_s)
    return sn, a, (int(max_a != 0 and bool((a != u).any())), int(max_s != 0 and bool((sn != raw).any())))


def run(real, Q, R, gamma, alpha, x0, noise, sim=None, threshold="step", ord=np.inf, l=0.0, eps_lc=0.0, dA=0.0,
        dB=0.0, thr_fixed=0.0, F0=None, V0=None):
    """real, sim: model() tuples (sim None: a plain run); noise [T, na]; threshold "step" | "fixed".  Returns a dict:
    states [T, ns], actions [T, na], rewards [T] and admitted [T] (1 admitted, 0 refused and repeating, 2 refused
    with nothing admitted yet: that row is not meaningful), F, V, state, the counters, and the run's smallest |td|
    and |cost - threshold| (the distances from a step's discontinuities), and in how many steps reset_inbound changed
    a value: clip_a_real, clip_s_real (admitted steps), clip_a_sim, clip_s_sim (every step of a safe run)."""
    Q, R = np.asarray(Q, dtype=np.float64), np.asarray(R, dtype=np.float64)
    ns, na = real[0].shape[1], real[1].shape[1]
    F = np.zeros((na, ns)) if F0 is None else np.array(F0, dtype=np.float64)
    V = np.zeros(ns) if V0 is None else np.array(V0, dtype=np.float64)
    s = np.array(x0, dtype=np.float64)
    T = len(noise)
    states, actions, rewards = np.zeros((T, ns)), np.zeros((T, na)), np.zeros(T)
    flags = np.zeros(T, dtype=np.uint8)
    last = (np.zeros(ns), np.zeros(na), 0.0)
    n_adm = n_viol = n_upd = 0
    min_td = min_gap = np.inf
    clips = np.zeros(4, dtype=np.int64)                          # a real, s real, a sim, s sim
    for t in range(T):
        fa = F @ s
        u = fa + noise[t]
        admitted = True
        if sim is not None:
            thr = thr_fixed if threshold == "fixed" else \
                l - eps_lc * (dA * np.linalg.norm(s, 2) + dB * np.linalg.norm(u, 2))
            s_sim, _, how = step_counted(sim, s, u)
            clips[2:] += how
            c = np.linalg.norm(s_sim, ord)
            min_gap = min(min_gap, abs(c - thr))
            admitted = bool(c <= thr)
        if admitted:
            sn, a, how = step_counted(real, s, u)
            clips[:2] += how
            r = -(sn @ Q @ sn + a @ R @ a)
            if sim is not None:
                c = np.linalg.norm(sn, ord)
                min_gap = min(min_gap, abs(c - l))
                n_viol += 0 if c <= l else 1
            td = r + gamma * (V @ sn ** 2) - V @ s ** 2
            min_td = min(min_td, abs(td))
            V = V + alpha * td * s ** 2
            if td > 0:
                F = F + alpha * np.outer(u - fa, s)
                n_upd += 1
            last = (s, a, r)
            s = sn
            n_adm += 1
        states[t], actions[t], rewards[t] = last
        flags[t] = 1 if admitted else (0 if n_adm else 2)
    return dict(states=states, actions=actions, rewards=rewards, admitted_flags=flags, F=F, V=V, state=s,
                admitted=n_adm, violations=n_viol, actor_updates=n_upd, min_td=min_td, min_gap=min_gap,
                clip_a_real=int(clips[0]), clip_s_real=int(clips[1]), clip_a_sim=int(clips[2]),
                clip_s_sim=int(clips[3]))


def run_case(case, envs, x0, noise):
    """The oracle on a golden case: the environments are built from `envs`' classes, the thresholds as the agents'
    constructors compute them."""
    if case["kind"] == "plain":
        real = make_env(envs, case["env"])
        return run(model(real), real.Q, real.R, case["gamma"], case["alpha"], x0, noise)
    extra = case.get("extra", ())
    real = make_env(envs, case["env"], case["theta"][0], extra)
    sim = make_env(envs, case["env"], case["theta"][1], extra)
    eps, l, L_c = epsilon_of(case), case["l"], 1
    if case["kind"] == "bounded":
        L_theta = sim.op_norm_der_A * np.sqrt(2) * real.max_s + sim.op_norm_der_B * np.sqrt(1) * real.max_a
    else:
        L_theta = np.linalg.norm(np.array([0.1, 0]))
    return run(model(real), real.Q, real.R, case["gamma"], case["alpha"], x0, noise, sim=model(sim),
               threshold="step" if case["kind"] == "se" else "fixed", l=l, eps_lc=eps * L_c,
               dA=sim.op_norm_der_A, dB=sim.op_norm_der_B, thr_fixed=l - eps * L_c * L_theta)


def reference_arrays(res):
    """The oracle's records cut down to what the reference's run() returns."""
    keep = np.flatnonzero(res["admitted_flags"] != 2)
    if keep.size == 0:
        return np.array([]), np.array([]), np.array([])
    f = keep[0]
    return res["states"][f:], res["actions"][f:], res["rewards"][f:]
