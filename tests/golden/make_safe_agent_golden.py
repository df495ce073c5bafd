#!/usr/bin/env python3
"""Generate tests/golden/safe_agent.npz and its data_path database tests/golden/safe_agent_db.npz from the
reference's ARSAgent with safe=True (ars/ars_agent.py:40-66, :144-182, :187-220).

Uses the stand-ins of make_golden.py (`gym`, `ray`, `cma` replaced by in-memory modules without arithmetic);
the reference runs unmodified.  Runs only where the reference is available.  Written are DATA only
(numpy.load(allow_pickle=False)); no reference source text is stored.

Cases (H = 200):
  a  n = 3, V1, N = 1, approximation branch, Threshold(1, 0.3, 0.001), warm-start policy
  b  as a with V2
  c  n = 5, V1, N = 1, exact branch (row kernel form; with V2 the first admitted update
     re-whitens so hard that every later direction is refused at any threshold)
  d  n = 2, V1, N = 1, approximation branch (lane kernel form)
  e  n = 3, V2, N = 4, threshold out of reach below (every direction admitted)
  f  n = 3, V2, N = 4, threshold out of reach above (every direction refused)
  g  n = 5, V2, N = 1, exact branch: the row form with V2 whitening; any refusal rate strictly between 0 and 1
  h  n = 3, V1, N = 1, exact branch with epsilon = -1e-5: the simulator threshold sits below the safety threshold,
     so some admitted real rollouts fall below it, which pins the violation count and the printed lines (the
     approximation branch only makes the simulator heavier, whose returns stay below the real ones here)
In a-d the threshold is the first candidate (quantiles of the simulator returns around the warm-start policy) that
refuses 30-70 % of the iterations; every simulator return is asserted more than 1e-6 away from sim_threshold.

Usage:  python tests/golden/make_safe_agent_golden.py
"""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
_mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mg)          # installs the stand-ins and puts the reference on sys.path

import ars.ars_agent as ref_agent  # noqa: E402  (reference module)
from ars.parameters import EnvParam, ARSParam, Threshold  # noqa: E402

H = 200
ITERS = 25                       # runTraining: 1 warm-up + n_iter = ITERS - 1
REAL = dict(l_i=0.8, m_i=1.2, k=10.2, h=1e-3)     # ars/safe_exploration.py:23-25
EPSILON = 1e-3
THRESH = (1.0, 0.3, 0.001)       # Threshold(K, A, B)
ALPHA, NU = 0.0075, 0.1
GLOBAL_SEED = 11                 # np.random.seed before construction (the approximation draw)
SEED = 3                         # the agent's own seed
MARGIN = 1e-6

# tag: (n, V1, N, branch, mode[, epsilon, Threshold])
#   mode: 'tune' (30-70 % refused) | 'partial' (some refused) | 'violate' (some real returns below threshold)
#         | 'below' | 'above'
CASES = {
    "a": (3, True, 1, "approx", "tune"),
    "b": (3, False, 1, "approx", "tune"),
    "c": (5, True, 1, "exact", "tune"),
    "d": (2, True, 1, "approx", "tune"),
    "e": (3, False, 4, "approx", "below"),
    "f": (3, False, 4, "approx", "above"),
    "g": (5, False, 1, "exact", "partial"),
    "h": (3, True, 1, "exact", "violate", -1e-5, THRESH),
}


def case(tag):
    """(n, V1, N, branch, mode, epsilon, Threshold args) of a case."""
    c = CASES[tag]
    return c[:5] + (c[5:] if len(c) > 5 else (EPSILON, THRESH))


class RecordingEnv(ref_agent.Environment):
    """The reference Environment; rollouts of the simulators the agent builds per direction are recorded."""
    sim_returns = []
    agent_built = False

    def __init__(self, env_param):
        super().__init__(env_param)
        self.is_sim = RecordingEnv.agent_built    # the real world is built in the constructor

    def rollout(self, policy, covariance=None, mean=None):
        out = super().rollout(policy, covariance=covariance, mean=mean)
        if self.is_sim:
            RecordingEnv.sim_returns.append(out[0])
        return out


ref_agent.Environment = RecordingEnv


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


def warm_policy(n):
    return np.random.RandomState(100 + n).uniform(-1.0, 1.0, (n - 1, 2 * n + 2))


def make_db(path):
    """A small real-world database (the reference's on-disk format, ars/database.py:36-37)."""
    ep = EnvParam("LeonSwimmer-RealWorld", n=3, H=20, **REAL, epsilon=EPSILON)
    env = ref_agent.Environment.__mro__[1](ep)
    pols, trajs = [], []
    for j in range(2):
        pol = warm_policy(3) * (0.5 + j)
        _, states = env.rollout(pol)
        pols.append(pol)
        trajs.append(states)
    savez_stable(path, dict(policies=np.array(pols), trajectories=np.array(trajs)))


def run(tag, threshold, db_path, w0_path):
    n, V1, N, branch, _, eps, thresh = case(tag)
    ep = EnvParam("LeonSwimmer-RealWorld", n=n, H=H, **REAL, epsilon=eps)
    ap = ARSParam("SafeGolden", V1=V1, n_iter=ITERS - 1, H=H, N=N, b=N, alpha=ALPHA, nu=NU, safe=True,
                  threshold=threshold, initial_w=w0_path)
    RecordingEnv.sim_returns = []
    RecordingEnv.agent_built = False
    np.random.seed(GLOBAL_SEED)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        agent = ref_agent.ARSAgent(ep, ap, data_path=db_path, seed=SEED,
                                   approx_error=eps if branch == "approx" else None,
                                   sim_thresh=Threshold(*thresh))
        RecordingEnv.agent_built = True
        per_it = []
        inner = agent.runOneIteration

        def recorded():
            r = inner()
            per_it.append(list(r))
            return r
        agent.runOneIteration = recorded
        curve = agent.runTraining()
    below = sum(1 for line in buf.getvalue().splitlines() if "below the threshold" in line)
    return agent, ep, per_it, np.array(curve), below, np.array(RecordingEnv.sim_returns)


def main():
    tmp = tempfile.mkdtemp()
    db_path = os.path.join(HERE, "safe_agent_db.npz")
    make_db(db_path)
    out = {}
    for tag in CASES:
        n, V1, N, branch, mode, eps, thresh = case(tag)
        alpha = Threshold(*thresh).compute_alpha(H)
        found = False
        for scale in (1.0, 0.3, 3.0):          # warm-start scale: the first that admits a candidate
            w0 = warm_policy(n) * scale
            w0_path = os.path.join(tmp, f"w0_{tag}.npy")
            np.save(w0_path, w0)
            if mode == "below":
                choices = [-1e9]
            elif mode == "above":
                choices = [1e9]
            else:
                # a refused iteration leaves the policy where it is: candidate simulator thresholds are quantiles
                # of the simulator returns around the warm-start policy (an all-refused run, r+ only)
                _, _, _, _, _, sims = run(tag, 1e9, db_path, w0_path)
                choices = [float(np.quantile(sims, q)) - alpha * eps
                           for q in (0.5, 0.6, 0.4, 0.7, 0.3, 0.2, 0.1)]
            for threshold in choices:
                agent, ep, per_it, curve, below, sims = run(tag, threshold, db_path, w0_path)
                refused = sum(1 for r in per_it if len(r) == 0) / len(per_it)
                margin_ok = bool(np.all(np.abs(sims - agent.sim_threshold) > MARGIN))
                ok = {"tune": 0.3 <= refused <= 0.7, "partial": 0.0 < refused < 1.0,
                      "violate": refused < 1.0 and below > 0}.get(mode, True)
                if ok and margin_ok:
                    found = True
                    break
                print(f"case {tag}: scale {scale} threshold {threshold:.6g} refuses {refused:.2f} "
                      f"(margin ok: {margin_ok})")
            if found:
                break
        if not found:
            raise SystemExit(f"case {tag}: no candidate threshold refuses 30-70 % of the iterations")
        assert np.all(np.abs(sims - agent.sim_threshold) > MARGIN), tag
        counts = np.array([len(r) for r in per_it], dtype=np.int64)
        rets = np.full((len(per_it), 2 * N), np.nan)
        for j, r in enumerate(per_it):
            rets[j, :len(r)] = r
        est = agent.estimated_param
        out[tag + "_cfg"] = np.array([n, int(V1), N, N, H, SEED, ITERS, GLOBAL_SEED,
                                      {"approx": 0, "exact": 1}[branch]], dtype=np.int64)
        out[tag + "_phys"] = np.array([REAL["l_i"], REAL["m_i"], REAL["k"], REAL["h"], eps, ALPHA, NU,
                                       threshold] + list(thresh))
        out[tag + "_w0"] = w0
        out[tag + "_counts"] = counts
        out[tag + "_returns"] = rets
        out[tag + "_curve"] = curve
        out[tag + "_policy"] = np.array(agent.policy)
        if not V1:
            out[tag + "_mean"] = np.array(agent.mean)
            out[tag + "_cov"] = np.array(agent.covariance)
        out[tag + "_sim_threshold"] = np.array(agent.sim_threshold)
        out[tag + "_estimated"] = np.array([est.l_i, est.m_i, est.k, est.h])
        out[tag + "_below"] = np.array(below, dtype=np.int64)
        print(f"case {tag}: threshold {threshold:.6g}, refused {np.mean(counts == 0):.2f}, "
              f"below-threshold lines {below}")
    savez_stable(os.path.join(HERE, "safe_agent.npz"), out)


if __name__ == "__main__":
    main()
