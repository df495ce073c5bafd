#!/usr/bin/env python3
"""Generate tests/golden/safe_experiment.npz from the reference's safe_ars/experiment.py: per seed a Basic_ARS and a
Safe_ARS agent trained from the same seed (`experience(seed)`, :46-68), the costs the script recomputes from the first
2 n_iter rollouts' states (:81-82) and the means it plots (:90-93).

Uses the stand-ins and the loader of make_golden.py; the reference's classes run unmodified (safe_ars/ars.py and the
Gym swimmer are loaded from the reference, the script's own statements -- which run at import and parse sys.argv --
are restated here line by line).  Runs only where the reference is available.  Written are DATA only
(numpy.load(allow_pickle=False)); no reference source text is stored.

Block a (the four agents the GPU tests train): n = 3, real swimmer (1, 1, 10), theta_sim = theta_real + u / ||u|| * 0.5
with u = RandomState(5).rand(3), cost max_i |thetadot_i|, real_thresh 0.502, sim_thresh 0.5, n_iter = 4, N = 4, b = 2,
alpha = 0.02, nu = 0.5, H = 50, seeds 3 and 4.
Block c (the script's use of NumPy's global generator): np.random.seed(0), n_seeds = 3, epsilon = 0.05, thresh = 1.5,
n_iter = 2, N = 2, b = 2, alpha = 0.02, nu = 0.5, H = 30: the drawn theta_sim, the three chained seeds, the four
means, and the next draw of the global generator behind the run.

Asserted, so that a test can neither pass by luck nor flip on rounding: every iteration of every safe agent of block a
has a refused and an unrefused rollout; every simulated cost the gate compared is at least 1e-9 from sim_thresh and
every real cost of a taken step at least 1e-9 from real_thresh, in both blocks.

Usage:  python tests/golden/make_safe_experiment_golden.py
"""
import contextlib
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
_mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mg)          # installs the stand-ins and puts the reference on sys.path

arsmod = _mg._load_by_path("ref_safe_ars", "safe_ars/ars.py")
SwimmerEnv = _mg.SwimmerEnv

N_SEG = 3
THETA_REAL = [1., 1., 10.]
MARGIN = 1e-9


def savez_stable(path, arrays):
    """np.savez_compressed without the wall-clock timestamps zipfile stamps on each member, so that a
    regeneration is byte-identical."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


class Probe(object):
    """The script's cost (experiment.py:44) as a callable that also keeps every value it returned, filed under the
    environment that stepped last (the simulator: a cost the gate compares; the real world: the cost of a taken
    step), and the real steps taken per rollout.  The values come out of the reference's own set_state + step."""

    def __init__(self, real_env, sim_env):
        self.seen = {"sim": [], "real": []}
        self.taken = []
        self.last = None
        for env, tag in ((real_env, "real"), (sim_env, "sim")):
            env.step = self._stepper(env.step, tag)
        inner_reset = real_env.reset

        def reset():
            self.taken.append(0)
            return inner_reset()
        real_env.reset = reset

    def _stepper(self, inner, tag):
        def step(action):
            self.last = tag
            if tag == "real":
                self.taken[-1] += 1
            return inner(action)
        return step

    def __call__(self, x):
        c = np.max([abs(x[3 + 2 * i]) for i in range(N_SEG)])
        if self.last is not None:
            self.seen[self.last].append(c)
        return c


def make_envs(theta_sim):
    real_env = SwimmerEnv("RealWorld", n=N_SEG, m_i=THETA_REAL[0], l_i=THETA_REAL[1], k=THETA_REAL[2])
    sim_env = SwimmerEnv("Simulator", n=N_SEG, m_i=theta_sim[0], l_i=theta_sim[1], k=theta_sim[2])
    return real_env, sim_env


def experience(seed, real_env, sim_env, cost, thresh, sim_thresh, n_iter, N, b, alpha, nu, H):
    """experiment.py:46-68, and the script's cost recomputation (:81-82) on what it returns."""
    unsafe_agent = arsmod.Basic_ARS()
    safe_agent = arsmod.Safe_ARS(cost, thresh, sim_thresh, sim_env)
    out = {}
    for kind, agent in (("unsafe", unsafe_agent), ("safe", safe_agent)):
        np.random.seed(seed)
        first = len(cost.taken)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            returns, states = agent.train(n_iter, real_env, N, b, alpha, nu, H)
        cost.last = None               # what follows is bookkeeping, not the gate
        out[kind + "_returns"] = returns
        out[kind + "_policy"] = np.array(agent.policy)
        out[kind + "_costs"] = np.array([cost(states[i, j]) for i in range(2 * n_iter) for j in range(H)])
        out[kind + "_cost_max"] = np.array([max(cost(s) for s in roll) for roll in states])
        out[kind + "_taken"] = np.array(cost.taken[first:], dtype=np.int64)
        out[kind + "_printed"] = sum(1 for line in buf.getvalue().splitlines() if "constraint not satisfied" in line)
    return out


def check_margins(cost, thresh, sim_thresh, what):
    sim, real = np.array(cost.seen["sim"]), np.array(cost.seen["real"])
    assert sim.size and real.size, what
    assert np.all(np.abs(sim - sim_thresh) >= MARGIN), f"{what}: a simulated cost within {MARGIN} of sim_thresh"
    assert np.all(np.abs(real - thresh) >= MARGIN), f"{what}: a real cost within {MARGIN} of real_thresh"


def block_a(out):
    thresh, sim_thresh = 0.502, 0.5
    n_iter, N, b, alpha, nu, H = 4, 4, 2, 0.02, 0.5, 50
    seeds = [3, 4]
    u = np.random.RandomState(5).rand(3)
    theta_sim = THETA_REAL + u / np.linalg.norm(u, ord=2) * 0.5
    real_env, sim_env = make_envs(theta_sim)
    cost = Probe(real_env, sim_env)
    runs = [experience(s, real_env, sim_env, cost, thresh, sim_thresh, n_iter, N, b, alpha, nu, H) for s in seeds]
    check_margins(cost, thresh, sim_thresh, "block a")
    for s, r in zip(seeds, runs):
        assert np.all(r["unsafe_taken"] == H)
        per_it = r["safe_taken"].reshape(n_iter, 2 * N)
        assert np.all((per_it < H).any(axis=1)) and np.all((per_it == H).any(axis=1)), \
            f"seed {s}: an iteration of the safe agent without a refused or without an unrefused rollout"
        # the unsafe agent's violations are not printed by the reference (Basic_ARS has no threshold)
        print(f"seed {s}: safe first-refused steps {sorted(set(per_it[per_it < H].tolist()))}, printed violations "
              f"{r['safe_printed']}, unsafe worst cost {r['unsafe_cost_max'].max():.4f}")
    out["a_cfg"] = np.array([N_SEG, n_iter, N, b, H], dtype=np.int64)
    out["a_hyper"] = np.array([alpha, nu, thresh, sim_thresh])
    out["a_seeds"] = np.array(seeds, dtype=np.int64)
    out["a_theta_real"] = np.array(THETA_REAL)
    out["a_theta_sim"] = np.array(theta_sim)
    for kind in ("unsafe", "safe"):
        for key in ("returns", "policy", "costs", "cost_max"):
            out[f"a_{kind}_{key}"] = np.array([r[f"{kind}_{key}"] for r in runs])
    out["a_safe_first_refused"] = np.array([r["safe_taken"] for r in runs])      # steps taken = first refused step
    out["a_safe_violations"] = np.array([r["safe_printed"] for r in runs], dtype=np.int64)


def block_c(out):
    epsilon, thresh, n_iter, N, b, alpha, nu, H, n_seeds = 0.05, 1.5, 2, 2, 2, 0.02, 0.5, 30, 3
    np.random.seed(0)
    delta = np.random.rand(len(THETA_REAL))                                     # experiment.py:36-37
    theta_sim = THETA_REAL + delta / np.linalg.norm(delta, ord=2) * epsilon
    real_env, sim_env = make_envs(theta_sim)
    cost = Probe(real_env, sim_env)
    seeds, acc = [], {k: [] for k in ("unsafe_returns", "unsafe_costs", "safe_returns", "safe_costs")}
    for _ in range(n_seeds):
        seed = np.random.randint(2**32 - 1)                                     # :77
        seeds.append(seed)
        r = experience(seed, real_env, sim_env, cost, thresh, thresh - 1, n_iter, N, b, alpha, nu, H)
        for k in acc:
            acc[k].append(r[k])
    out["c_next_draw"] = np.array(np.random.randint(2**32 - 1), dtype=np.int64)  # where the script leaves the generator
    check_margins(cost, thresh, thresh - 1, "block c")
    out["c_cfg"] = np.array([N_SEG, n_iter, N, b, H, n_seeds, 0], dtype=np.int64)
    out["c_hyper"] = np.array([alpha, nu, thresh, epsilon])
    out["c_theta_sim"] = np.array(theta_sim)
    out["c_seeds"] = np.array(seeds, dtype=np.int64)
    for k, v in acc.items():
        out["c_mean_" + k] = np.mean(v, axis=0)                                 # :90-93
    print("block c: theta_sim", theta_sim, "seeds", seeds)


def main():
    out = {}
    block_a(out)
    block_c(out)
    path = os.path.join(HERE, "safe_experiment.npz")
    savez_stable(path, out)
    print("safe_experiment.npz", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
