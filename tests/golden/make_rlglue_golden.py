#!/usr/bin/env python3
"""Generate tests/golden/rlglue_ars.npz from the reference's own SwimmerARSAgent (rlglue/agent/SwimmerAgent.py).

The agent runs unmodified.  The four `rlglue` codec modules it imports (rlglue.agent.Agent, rlglue.agent.AgentLoader,
rlglue.types, rlglue.utils.TaskSpecVRLGLUE3) are replaced by in-memory stand-ins without arithmetic; the task-spec
string is the one the environment sends (SwimmerEnvironment.cpp:30, std::to_string formatting); the agent reads its own
`../parameters.txt` from a temporary working directory; the experiment program's loop (SwimmerExperiment.cpp:65-84:
"load state" every H steps, RL_step, freeze / unfreeze, "get total_reward") drives it on the CPU oracle's twin step
(oracle.swimmer_oracle.twin_step).  Runs only where the reference is available.  Written are DATA only
(numpy.load(allow_pickle=False)); no reference source text is stored.

Per case <tag>_*: params [seed, n, N, b, H, alpha, nu, max_u, h, iterations, l_i, k, m_i, dir_x, dir_y]; deltas
[iterations + 1][N][m][d] (a replay of NumPy's stream: agent_start's draw, then the one after every iteration);
eval [iterations] (the lines of results.txt); policies [iterations][m][d] (after every update); rew [iterations][2N]
(`rewards` as update_policy saw it, recorded through a subclass); clips [3] (action components clipped high, clipped
low, inside, over every select_action); next_rand (np.random.rand() after the run: the stream position); and
sens_eval, sens_rew, sens_policies: the REFERENCE'S OWN SENSITIVITY, the largest change of each quantity over 8 reruns
in which every new state is multiplied by 1 + 1e-13 U(-1, 1) per component (1e-13 stands for the documented <= 8e-14
distance between the device twin step and the dense oracle).

Conditions asserted here, on the reference alone: every sensitivity > 0; with b = 1, |r+ - r-| >= 1e6 x the returns'
sensitivity, so a sign cannot flip; policy sensitivity <= 1e-7; in the clip cases each of high / low / inside holds at
least 10 % of the action components.  The H = 1 case (G) is the exception, because the reference does not survive
H = 1: every return is the same number there (run_case says why), sigma is 0, and the first update leaves an all-NaN
policy.  G records that one iteration -- equal returns, NaN policy, evaluation return 0 -- and the conditions on
returns' gaps and on the policy's and the evaluation's sensitivity do not apply to it.

Usage:  python tests/golden/make_rlglue_golden.py
"""
import contextlib
import importlib.util
import io
import os
import re
import sys
import tempfile
import types
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SWIMMER_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

import oracle  # noqa: E402

START = 0.001
RERUNS = 8
# tag: (seed, n, N, b, H, alpha, nu, max_u, h, iterations); l_i, k, m_i, direction: the shipped file's
CASES = {
    "A": (0, 3, 1, 1, 10, 0.02, 0.05, 5.0, 0.01, 6),
    "B": (1, 2, 2, 2, 20, 0.02, 0.05, 5.0, 0.01, 5),
    "C": (2, 4, 3, 2, 15, 0.05, 0.1, 5.0, 0.01, 4),
    "D": (3, 5, 2, 1, 40, 0.02, 0.05, 5.0, 0.01, 4),
    "E": (4, 6, 3, 1, 2, 0.02, 2.0, 5.0, 0.01, 6),
    "F": (5, 8, 2, 2, 12, 0.02, 0.05, 5.0, 0.01, 4),
    "G": (7, 3, 2, 1, 1, 0.02, 2.0, 5.0, 0.01, 1),                # H = 1: the reference's first update is 0 / 0
    "SHIPPED": (9, 3, 1, 1, 1000, 0.02, 0.02, 5.0, 0.01, 3),      # rlglue/parameters.txt
    "CLIP1": (6, 3, 2, 2, 40, 0.05, 0.3, 5e-4, 0.01, 6),
    # max_u 1e-3: at 5e-4 this run has 1242 / 847 / 164, "inside" below the 10 % every class must hold
    "CLIP2": (8, 4, 2, 1, 30, 0.05, 0.5, 1e-3, 0.01, 5),
}
L_I, K, M_I, DIRECTION = 1.0, 10.0, 1.0, (1.0, 0.0)


def _install_standins():
    class Agent(object):
        pass

    class _Doubles(object):
        def __init__(self, numInts=None, numDoubles=None, numChars=None):
            self.intArray, self.charArray = [], []
            self.doubleArray = [0.0] * (numDoubles or 0)

    class Action(_Doubles):
        pass

    class Observation(_Doubles):
        pass

    class TaskSpecParser(object):
        """What the agent asks of the RL-Glue task-spec parser: the action and the observation ranges."""

        def __init__(self, spec):
            spec = spec.decode() if isinstance(spec, bytes) else spec
            obs = re.search(r"OBSERVATIONS DOUBLES \((\d+) (\S+) (\S+)\)", spec)
            act = re.search(r"ACTIONS DOUBLES \((\d+) (\S+) (\S+)\)", spec)
            self.valid = bool(obs and act)
            self._obs = [[obs.group(2), obs.group(3)]] * int(obs.group(1))
            self._act = [[float(act.group(2)), float(act.group(3))]] * int(act.group(1))

        def getDoubleActions(self):
            return self._act

        def getDoubleObservations(self):
            return self._obs

    mods = {name: types.ModuleType(name) for name in
            ("rlglue", "rlglue.agent", "rlglue.agent.Agent", "rlglue.agent.AgentLoader", "rlglue.types", "rlglue.utils",
             "rlglue.utils.TaskSpecVRLGLUE3")}
    mods["rlglue.agent.Agent"].Agent = Agent
    mods["rlglue.agent.AgentLoader"].loadAgent = lambda agent: None
    mods["rlglue.types"].Action, mods["rlglue.types"].Observation = Action, Observation
    mods["rlglue.utils.TaskSpecVRLGLUE3"].TaskSpecParser = TaskSpecParser
    mods["rlglue"].agent, mods["rlglue"].types, mods["rlglue"].utils = (mods["rlglue.agent"], mods["rlglue.types"],
                                                                        mods["rlglue.utils"])
    mods["rlglue.agent"].Agent, mods["rlglue.agent"].AgentLoader = (mods["rlglue.agent.Agent"],
                                                                    mods["rlglue.agent.AgentLoader"])
    mods["rlglue.utils"].TaskSpecVRLGLUE3 = mods["rlglue.utils.TaskSpecVRLGLUE3"]
    sys.modules.update(mods)
    spec = importlib.util.spec_from_file_location("SwimmerAgent", os.path.join(REF, "rlglue/agent/SwimmerAgent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, Observation


ref, Observation = _install_standins()


def task_spec(n, max_u):
    # SwimmerEnvironment.cpp:30; std::to_string(double) is "%f"
    return ("VERSION RL-Glue-3.0 PROBLEMTYPE continuing DISCOUNTFACTOR 0.9 OBSERVATIONS DOUBLES (%d UNSPEC UNSPEC) "
            "ACTIONS DOUBLES (%d %f %f) REWARDS (UNSPEC UNSPEC) EXTRA SwimmerEnvironment(C++) by Leon Zheng"
            % (2 * n + 2, n - 1, -max_u, max_u)).encode()


def run_reference(seed, n, N, b, H, alpha, nu, max_u, h, iterations, perturb=None):
    """One run of the experiment program's loop; perturb: None or state -> state on every new state."""
    rec = dict(rew=[], policies=[], clips=np.zeros(3, dtype=np.int64))

    class Recording(ref.SwimmerARSAgent):
        def update_policy(self, order):
            rec["rew"].append(list(self.rewards))
            super().update_policy(order)
            rec["policies"].append(self.agentPolicy.copy())

        def select_action(self, policy, state):
            raw = np.matmul(policy, np.array(state.doubleArray))     # a second look: draws nothing, changes nothing
            rec["clips"] += [int((raw > self.max_u).sum()), int((raw < -self.max_u).sum()),
                             int((~(raw > self.max_u) & ~(raw < -self.max_u)).sum())]     # a NaN is in neither branch: passes
            return super().select_action(policy, state)

    p = oracle.OracleParams.make(n, L_I, M_I, K, h, DIRECTION)
    keep = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.mkdir(os.path.join(tmp, "agent"))
        with open(os.path.join(tmp, "parameters.txt"), "w") as f:
            f.write(f"n_seg {n}\ndirection {DIRECTION[0]!r} {DIRECTION[1]!r}\nh_global {h!r}\nN {N}\nb {b}\nH {H}\n"
                    f"alpha {alpha!r}\nnu {nu!r}\nmax_u {max_u!r}\nl_i {L_I!r}\nk {K!r}\nm_i {M_I!r}\n")
        os.chdir(os.path.join(tmp, "agent"))
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                np.random.seed(seed)
                agent = Recording()
                agent.agent_message(b"set parameters")
                agent.agent_init(task_spec(n, max_u))
                saved = [START] * (2 * n + 2)                                  # env_start + save_state
                state = list(saved)

                def obs_of(s):
                    o = Observation(numDoubles=len(s))
                    o.doubleArray = list(s)
                    return o

                def rl_step(state, action):
                    nxt, r = oracle.twin_step(p, np.array(state), np.array(action.doubleArray))
                    if perturb is not None:
                        nxt = perturb(nxt)
                    return list(nxt), agent.agent_step(r, obs_of(nxt))

                action = agent.agent_start(obs_of(state))
                evals = []
                for _ in range(iterations):                                    # runOneTrainingIteration
                    agent.agent_message(b"unfreeze training")
                    for i in range(2 * H * N):
                        if i % H == 0:
                            state = list(saved)                                # "load state"
                        state, action = rl_step(state, action)
                    agent.agent_message(b"freeze training")
                    state = list(saved)
                    for i in range(H):
                        state, action = rl_step(state, action)
                    evals.append(float(agent.agent_message(b"get total_reward")))
                next_rand = np.random.rand()
        finally:
            os.chdir(keep)
    return dict(eval=np.array(evals), rew=np.array(rec["rew"]), policies=np.array(rec["policies"]),
                clips=rec["clips"], next_rand=np.float64(next_rand))


def relative_noise(seed, scale=1e-13):
    rs = np.random.RandomState(seed)               # a generator of its own: the agent's is NumPy's global one
    return lambda s: s * (1.0 + scale * (2.0 * rs.rand(len(s)) - 1.0))


def run_case(tag, case):
    seed, n, N, b, H, alpha, nu, max_u, h, iterations = case
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        base = run_reference(*case)
    m, d = n - 1, 2 * n + 2
    deltas = np.random.RandomState(seed).rand(iterations + 1, N, m, d)
    rs = np.random.RandomState(seed)
    rs.rand(iterations + 1, N, m, d)
    assert rs.rand() == base["next_rand"], "the run's draws are not the first (iterations + 1) N m d of the stream"
    # H = 1: the reward of the one step from the start state does not depend on the action (the torques reach Gdot a
    # step later), so every entry of rew is the same number, sigma is 0 and the first update is 0 / 0: the reference
    # leaves an all-NaN policy (a RuntimeWarning) and raises in the next iteration's stdev.  That IS its H = 1 run; the
    # case records its one iteration, and the policy's sensitivity is not defined
    diverges = not np.isfinite(base["policies"]).all()
    assert diverges == (H == 1), (tag, base["policies"])
    sens = dict(eval=0.0, rew=0.0, policies=0.0)
    for r in range(RERUNS):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            got = run_reference(*case, perturb=relative_noise(1000 + r))
        for key in sens:
            if diverges and key == "policies":
                assert np.array_equal(np.isnan(got[key]), np.isnan(base[key]))
                continue
            sens[key] = max(sens[key], float(np.abs(got[key] - base[key]).max()))
    if diverges:
        # every step starts from the exact start state, so perturbing the NEW states moves nothing: the returns'
        # sensitivity is taken as what the perturbation stands for, 1e-13 relative, applied to the return itself
        assert np.isnan(base["policies"]).all() and sens["rew"] == 0 and (base["rew"] == base["rew"][0, 0]).all()
        sens["rew"] = 1e-13 * abs(float(base["rew"][0, 0]))
    else:
        assert sens["rew"] > 0 and sens["policies"] > 0 and sens["eval"] > 0, (tag, sens)
        assert sens["policies"] <= 1e-7, (tag, sens)
    if b == 1 and not diverges:
        gap = np.abs(base["rew"][:, 0] - base["rew"][:, 1]).min()
        assert gap >= 1e6 * sens["rew"], (tag, gap, sens)
    if tag.startswith("CLIP"):
        assert base["clips"].min() >= 0.1 * base["clips"].sum(), (tag, base["clips"])
    print(tag, case, "eval", base["eval"], "clips", base["clips"], "sens", sens)
    out = dict(params=np.array([seed, n, N, b, H, alpha, nu, max_u, h, iterations, L_I, K, M_I, *DIRECTION]),
               deltas=deltas, eval=base["eval"], policies=base["policies"], rew=base["rew"], clips=base["clips"],
               next_rand=base["next_rand"], sens_eval=np.float64(sens["eval"]), sens_rew=np.float64(sens["rew"]),
               sens_policies=np.float64(sens["policies"]))
    return {f"{tag}_{k}": v for k, v in out.items()}


if __name__ == "__main__":
    out = {}
    for tag, case in CASES.items():
        out.update(run_case(tag, case))
    path = os.path.join(HERE, "rlglue_ars.npz")
    # np.savez stamps every member with the time of day; fixed stamps make a regeneration byte-identical
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, value in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       zipfile.ZIP_DEFLATED)
    print("wrote", path, os.path.getsize(path), "bytes")
