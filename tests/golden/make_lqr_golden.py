#!/usr/bin/env python3
"""Generate tests/golden/lqr.npz from the reference's own LQR agents (cacla/cacla_agent.py CACLA_LQR_agent,
cacla/cacla_safe_agent.py) on its own environments (envs/gym_lqr/lqr_env.py), and from its window_convolution.

Uses the stand-ins of make_golden.py (`gym`, `ray`, `cma` replaced by in-memory modules without arithmetic); the
reference runs unmodified.  Runs only where the reference is available.  Written are DATA only
(numpy.load(allow_pickle=False)); no reference source text is stored.

The cases are tests/lqr_oracle.py's CASES (the table of the issue): per case, after np.random.seed(seed), the
hyper-parameters, the three returned arrays, the final F, V and environment state, the counters (admitted steps =
calls of backward_value_FA, actor updates = calls of backward_action_FA, violations = the real constraint's
unsatisfied checks, counted through a Constraint subclass that only looks), the replayed initial state and noise
(NumPy's stream again from the same seed) and the next np.random.standard_normal() after the run -- the witness of how
much of the global stream the run consumed.

Besides: per environment class a short sequence of hand-driven transitions (env_*), bounds and drift included, and a
window_convolution of 300 values with H = 50.

Tie condition: a faithful implementation can legitimately differ only where temp_diff lies within rounding of 0 or a
cost within rounding of its threshold; every case is asserted to keep |temp_diff| and |cost - threshold| >= 1e-6.

Usage:  python tests/golden/make_lqr_golden.py
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
_mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mg)          # installs the stand-ins and puts the reference on sys.path
_spec = importlib.util.spec_from_file_location("lqr_oracle", os.path.join(HERE, "..", "lqr_oracle.py"))
lqr_oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lqr_oracle)

import cacla.cacla_agent as ref_agent  # noqa: E402  (reference modules)
import cacla.cacla_safe_agent as ref_safe  # noqa: E402
import cacla.window as ref_window  # noqa: E402
import envs.gym_lqr.lqr_env as ref_envs  # noqa: E402

MARGIN = 1e-6


def run_case(case):
    seen = dict(min_td=np.inf, min_gap=np.inf, admitted=0, actor_updates=0, violations=0)

    class Constraint(ref_safe.Constraint):
        real = False

        def satisfied(self, state):
            ok = super().satisfied(state)
            seen["min_gap"] = min(seen["min_gap"], abs(float(self.cost(state)) - self.l))
            if self.real and not ok:
                seen["violations"] += 1
            return ok

    keep = ref_safe.Constraint
    ref_safe.Constraint = Constraint         # the per-step simulator constraints are made of the module's class
    try:
        agent, real, sim = lqr_oracle.build(case, ref_envs, ref_agent.CACLA_LQR_agent, ref_safe, Constraint)
        if case["kind"] != "plain":
            agent.constraint.real = True
        value_fa, action_fa = agent.backward_value_FA, agent.backward_action_FA

        def backward_value_FA(alpha, delta, state):
            seen["min_td"] = min(seen["min_td"], abs(float(delta)))
            seen["admitted"] += 1
            return value_fa(alpha, delta, state)

        def backward_action_FA(*a):
            seen["actor_updates"] += 1
            return action_fa(*a)
        agent.backward_value_FA, agent.backward_action_FA = backward_value_FA, backward_action_FA
        np.random.seed(case["seed"])
        with contextlib.redirect_stdout(io.StringIO()):
            states, actions, rewards = agent.run(case["steps"], case["gamma"], case["alpha"], case["sigma"],
                                                 H=10 ** 9)
        next_normal = np.random.standard_normal()
    finally:
        ref_safe.Constraint = keep
    ns, na = agent.F.shape[1], agent.F.shape[0]
    np.random.seed(case["seed"])             # the replay: rand(ns), then steps * na normals
    x0 = np.random.rand(ns)
    noise = np.random.multivariate_normal(np.zeros(na), case["sigma"] * np.identity(na), size=case["steps"])
    assert np.random.standard_normal() == next_normal
    assert seen["min_td"] >= MARGIN and seen["min_gap"] >= MARGIN, seen
    hyper = [case["seed"], case["steps"], case["gamma"], case["alpha"], case["sigma"], case.get("l", 0.0)]
    return dict(hyper=np.array(hyper, dtype=np.float64), states=np.array(states, dtype=np.float64),
                actions=np.array(actions, dtype=np.float64), rewards=np.array(rewards, dtype=np.float64),
                F=np.array(agent.F), V=np.array(agent.V), state=np.array(real.state, dtype=np.float64),
                counters=np.array([seen["admitted"], seen["violations"], seen["actor_updates"]], dtype=np.int64),
                x0=x0, noise=noise, next_normal=np.float64(next_normal),
                margins=np.array([seen["min_td"], seen["min_gap"]]))


def env_transitions(out):
    """Hand-driven steps of every environment class: large actions and states so that both bounds act."""
    rs = np.random.RandomState(7)
    made = {"LinearQuadReg": lqr_oracle.make_env(ref_envs, "p13"),
            "EasyParamLinearQuadReg": ref_envs.EasyParamLinearQuadReg(0.9),
            "BoundedEasyLinearQuadReg": ref_envs.BoundedEasyLinearQuadReg(0.95, 1.0, 0.5),
            "BoundedActionEasyLinearQuadReg": ref_envs.BoundedActionEasyLinearQuadReg(0.95, 1.0),
            "EasyAffineQuadReg": ref_envs.EasyAffineQuadReg(0.99)}
    for name, env in made.items():
        ns, na = env.observation_space.shape[0], env.action_space.shape[0]
        s0 = rs.uniform(-1.5, 1.5, ns)
        acts = rs.normal(0.0, 1.0, (16, na))
        env.set_state(s0.copy())
        states, rewards, taken = [], [], []
        for u in acts:
            obs, rew, done, info = env.step(u.copy())
            states.append(np.array(obs))
            rewards.append(rew)
            taken.append(np.array(info["action"]))
        out[f"env_{name}_s0"], out[f"env_{name}_u"] = s0, acts
        out[f"env_{name}_states"], out[f"env_{name}_rewards"] = np.array(states), np.array(rewards, dtype=np.float64)
        out[f"env_{name}_actions"] = np.array(taken)


if __name__ == "__main__":
    out = {}
    for tag, case in lqr_oracle.CASES.items():
        res = run_case(case)
        print(tag, "arrays", res["states"].shape, "admitted/violations/updates", res["counters"],
              "min |temp_diff| %.3g  min |cost - threshold| %.3g" % tuple(res["margins"]))
        for k, v in res.items():
            out[f"{tag}_{k}"] = v
    env_transitions(out)
    a = np.random.RandomState(3).normal(-1.0, 0.5, 300)
    out["window_a"], out["window_H"] = a, np.int64(50)
    out["window_out"] = np.asarray(ref_window.window_convolution(a, 50), dtype=np.float64)
    path = os.path.join(HERE, "lqr.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 300 * 1024
