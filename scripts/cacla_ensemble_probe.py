"""Does the step time of the ensemble gate of CACLA on the swimmer depend on the number of members?  The ensemble
kernel (sw_cacla_safe_ensemble_run_f64: the members ride in the lanes of the agent's wave) beside the single-simulator
one (sw_cacla_safe_run_f64), kernel only, from HIP events around one launch of 4096 steps with the noise already on
the device, in the same process on the same box -- 960 agents (one wave each; the reference's grid), n = 3 and n = 6
(two hidden units per lane), the gate open (infinite threshold: look-ahead, cost, real step and update at every step
-- the most a step can cost).

Per n: the single-simulator kernel and the ensemble kernel with E = 1, 8 and 64 members, with and without worst_rec
(the wave-wide maximum sits behind a uniform branch), timed ALTERNATELY -- one launch of each per repeat, so a drift
of the box falls on all of them alike.  ns per agent-step = launch time / steps: the agents' waves run side by side.

Medians of 5 after two warm-up rounds, with min .. max.   python scripts/cacla_ensemble_probe.py"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swimmer_amd as sw  # noqa: E402
from swimmer_amd import cacla  # noqa: E402
from swimmer_amd.cacla import safe_kernels  # noqa: E402

DEV = "cuda:0"
REPS, WARM, STEPS, AGENTS = 5, 2, 4096, 960
SIM = (1.02, 0.97, 10.3)
MEMBERS = (1, 8, 64)


def timed_alternately(launches):
    """{label: launch} -> {label: [ms] * REPS}: every repeat runs each launch once, in the given order."""
    ms = {label: [] for label in launches}
    for rep in range(REPS + WARM):
        for label, launch in launches.items():
            fresh = launch(None)                         # clones of the start state, outside the timed region
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(fresh)
            e1.record()
            torch.cuda.synchronize()
            if rep >= WARM:
                ms[label].append(e0.elapsed_time(e1))
    return ms


def row(label, ms):
    per = [x / STEPS * 1e6 for x in ms]
    print(f"    {label:<40} ms  median {statistics.median(ms):8.4f}  min {min(ms):8.4f}  max {max(ms):8.4f}   "
          f"ns per agent-step  median {statistics.median(per):7.1f}  ({min(per):.1f} .. {max(per):.1f})", flush=True)
    return statistics.median(per), min(per), max(per)


def members(E):
    """E simulators around SIM, the first SIM itself: distinct constants in the lanes."""
    rs = np.random.RandomState(E)
    rows = np.array(SIM) + np.concatenate([np.zeros((1, 3)), 0.01 * rs.standard_normal((E - 1, 3))])
    return np.tile(rows[None], (AGENTS, 1, 1))


def probe(n):
    A = AGENTS
    p = sw.SwParams.make(n)
    f64 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=DEV)   # noqa: E731
    w0 = f64(np.stack([cacla.draw_networks(n, torch.Generator().manual_seed(k)) for k in range(A)]))
    s0 = f64(np.tile(np.array(sw.SwimmerEnv(n=n).reset()), (A, 1)))
    gam, alp = f64(np.full(A, 0.9)), f64(np.full(A, 0.001))
    noise = torch.randn(A, STEPS, n - 1, dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(n))
    rewards = torch.empty(A, STEPS, dtype=torch.float64, device=DEV)
    rec = torch.empty(A, STEPS, dtype=torch.int32, device=DEV)
    worst = torch.empty(A, STEPS, dtype=torch.float64, device=DEV)
    gated = torch.ones(A, dtype=torch.int32, device=DEV)
    sim_thr, real_thr = f64(np.full(A, np.inf)), f64(np.full(A, 0.05))
    kind = sw._lib.COST_MAX_ABS_THETADOT

    def start():
        return (w0.clone(), s0.clone(), torch.full((A,), float("nan"), dtype=torch.float64, device=DEV),
                torch.zeros((A, 3), dtype=torch.int32, device=DEV), torch.full((A,), -1, dtype=torch.int32, device=DEV))

    sim1 = f64(np.tile(SIM, (A, 1)))

    def single(fresh):
        if fresh is None:
            return start()
        w, s, last, counters, first = fresh
        safe_kernels.cacla_safe_run(p, STEPS, 0, gam, alp, noise, gated, sim1, sim_thr, real_thr, kind, 0, w, s, last,
                                    counters, first, rewards=rewards, admitted_rec=rec)

    def ensemble(E, with_worst):
        sims = f64(members(E))
        refusals = torch.zeros((A, E), dtype=torch.int32, device=DEV)

        def launch(fresh):
            if fresh is None:
                return start()
            w, s, last, counters, first = fresh
            safe_kernels.cacla_safe_ensemble_run(p, STEPS, 0, gam, alp, noise, gated, sims, sim_thr, real_thr, kind, 0,
                                                 w, s, last, counters, first, rewards=rewards, admitted_rec=rec,
                                                 worst_rec=worst if with_worst else None, member_refusals=refusals)
        return launch

    launches = {"single-simulator kernel": single}
    for E in MEMBERS:
        launches[f"ensemble kernel, E = {E:2d}"] = ensemble(E, False)
        launches[f"ensemble kernel, E = {E:2d}, worst_rec"] = ensemble(E, True)
    print(f"n = {n}, {A} agents x {STEPS} steps, gate open", flush=True)
    ms = timed_alternately(launches)
    per = {label: row(label, ms[label]) for label in launches}
    base = per["single-simulator kernel"][0]
    for with_worst in ("", ", worst_rec"):
        e1 = per[f"ensemble kernel, E =  1{with_worst}"]
        e64 = per[f"ensemble kernel, E = 64{with_worst}"]
        print(f"        E = 1{with_worst}: {e1[0] / base:.3f} x the single-simulator step;  E = 64 / E = 1: "
              f"{e64[0] / e1[0]:.3f}  (repeats of E = 1 spread {e1[2] / e1[1]:.3f}, of E = 64 {e64[2] / e64[1]:.3f})",
              flush=True)


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0), flush=True)
    for n in (3, 6):
        probe(n)
