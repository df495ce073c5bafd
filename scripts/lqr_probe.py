"""CACLA on LQR (sw_lqr_cacla_run_f64, one agent per lane) on one GPU: what a run costs.

  (a) kernel only, from HIP events around the launch with the noise already on the device: ns per agent-step and per
      step of the chain at A = 1, 64, 960 and 16384 agents and two step counts (is the time linear in the steps, and
      flat in A while the waves have SIMDs to themselves?), for the plain agent without and with the per-step
      records and for the safe agent (per-step threshold) without records; the 2 x 1 problem of the reference;
  (b) end to end, the reference's two scripts as this package runs them: cacla.lqr_experiment.sweep (9 step sizes x
      200 000 steps, rewards kept, smoothed curves) and cacla.safe_exploration_lqr.compare (the plain and the safe
      agent, 20 000 steps each, everything kept), host draws, uploads, launches and copies back included;
  (c) end to end, a batch the reference has no counterpart of: 960 safe agents x 20 000 steps, nothing recorded.

Medians of 5 after a warm-up, with min .. max.   python scripts/lqr_probe.py"""
import contextlib
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swimmer_amd as sw  # noqa: E402
from swimmer_amd import cacla  # noqa: E402
from swimmer_amd.cacla import lqr  # noqa: E402
from swimmer_amd.envs.gym_lqr import lqr_env  # noqa: E402

DEV = "cuda:0"
REPS = 5


def stats(xs):
    return f"median {statistics.median(xs):.4g}  min {min(xs):.4g}  max {max(xs):.4g}"


def kernel_only(kind, A, steps, records):
    K = sw.kernels
    real, sim = lqr_env.EasyParamLinearQuadReg(0.9), lqr_env.EasyParamLinearQuadReg(0.85)
    con = cacla.Constraint(cacla.norm_cost(np.inf), 1.5, 1)
    col, cost = lqr.agent_column(kind, real, 0.9, 1e-3, sim, 0.05, con)
    params = torch.as_tensor(np.tile(col[:, None], (1, A)), device=DEV)
    noise = torch.randn(steps, 1, A, dtype=torch.float64, device=DEV) * 0.3
    x0 = torch.rand(2, A, dtype=torch.float64, device=DEV)
    rec = dict(rec_state=torch.empty(steps, 2, A, dtype=torch.float64, device=DEV),
               rec_action=torch.empty(steps, 1, A, dtype=torch.float64, device=DEV),
               rec_reward=torch.empty(steps, A, dtype=torch.float64, device=DEV),
               rec_admitted=torch.empty(steps, A, dtype=torch.uint8, device=DEV)) if records else {}
    ms = []
    for rep in range(REPS + 2):
        F = torch.zeros(1, 2, A, dtype=torch.float64, device=DEV)
        V = torch.zeros(2, A, dtype=torch.float64, device=DEV)
        s, last = x0.clone(), torch.zeros(4, A, dtype=torch.float64, device=DEV)
        counters = torch.zeros(3, A, dtype=torch.int32, device=DEV)
        status = torch.zeros(A, dtype=torch.int32, device=DEV)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        K.lqr_cacla_run(2, 1, steps, kind != "plain", K.LQR_THRESHOLD_STEP, cost, params, noise, F, V, s, last, counters,
                        status, **rec)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms[2:])
    print(f"(a) {kind:5s} {'records' if records else 'no rec.'}  A = {A:5d}  steps = {steps:5d}: ms  {stats(ms[2:])}   "
          f"{med * 1e6 / steps:8.1f} ns per step of the chain, {med * 1e6 / steps / A:9.3f} ns per agent-step   "
          f"(admitted {int(counters[0].sum())} of {A * steps}, status {int(status.max())})")
    return med


def timed(what, fn):
    out = []
    for rep in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    print(f"{what}: s  {stats(out[1:])}")
    return res


def main():
    print(torch.cuda.get_device_name(0))
    for kind, records in (("plain", False), ("plain", True), ("se", False)):
        for A in (1, 64, 960, 16384):
            t = [kernel_only(kind, A, steps, records) for steps in (2048, 8192)]
            print(f"      steps x 4 -> time x {t[1] / t[0]:.2f}")
    res = timed("(b) lqr_experiment.sweep, 9 step sizes x 200 000 steps, end to end", lambda: cacla.lqr_experiment.sweep())
    print("      distance to the optimal policy per step size:", " ".join(f"{d:.3g}" for d in res["distance"]))

    def batch_only():
        b = cacla.CACLA_LQR_Batch(cacla.lqr_experiment.lqr_2(), 1, list(cacla.lqr_experiment.ALPHAS), 0.1, range(9))
        return b.run(200000, record=("rewards",))
    timed("      of which CACLA_LQR_Batch.run (draws, uploads, launches, rewards back)", batch_only)
    res = timed("(b) safe_exploration_lqr.compare, 2 agents x 20 000 steps, end to end",
                lambda: cacla.safe_exploration_lqr.compare())
    print(f"      safe agent: admitted {res['safe']['admitted']} of 20000, violations {res['safe']['violations']}")

    A = 960
    k = np.arange(A)
    theta_sim = np.linspace(0.8, 0.99, 32)[k % 32]
    reals = lqr_env.EasyParamLinearQuadReg(1.0)
    sims = [lqr_env.EasyParamLinearQuadReg(t) for t in theta_sim]
    alphas = np.array([1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5])[(k // 32) % 6]

    def many():
        b = cacla.CACLA_LQR_Batch(reals, 1, alphas, 0.1, k, sim_envs=sims, epsilons=np.abs(1.0 - theta_sim),
                                  constraints=cacla.Constraint(cacla.norm_cost(np.inf), 4, 1), agent="se")
        b.run(20000, record=())
        return b
    b = timed(f"(c) {A} safe agents (32 simulator errors x 6 step sizes x 5 seeds) x 20 000 steps, no records, end to end", many)
    print(f"      admitted {int(b.admitted.min())} .. {int(b.admitted.max())}, violations {int(b.violations.sum())}, "
          f"status {int(b.status.max())}")


if __name__ == "__main__":
    main()
