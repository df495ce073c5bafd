"""Does the step time of the safe-ARS rollouts gated on an ensemble of simulators depend on the number of members?  The
ensemble kernel (sw_safe_ars_rollouts_ensemble_f64: a rollout in a group of lanes, a member per lane) beside the
existing lane-form kernel with one simulator per agent (sw_safe_ars_rollouts_multi_f64 under SW_FLAG_ROLLOUT_LANE) on
the same inputs, kernel only, from HIP events around one launch, in the same process on the same box -- the batch of
safe_ars/experiment.py at ten seeds: 20 agents x 16 rollouts x H = 1000, all gated, n = 3 and n = 6, the gate open
(infinite threshold: look-ahead, cost and real step at every step -- the most a step can cost).

Per n: the lane-form kernel and the ensemble kernel with E = 1, 8 and 64 members, with and without its two records
(worst_max, refusing_members), timed ALTERNATELY -- one launch of each per repeat, so a drift of the box falls on all of
them alike.  ns per step = launch time / H: the rollouts run side by side.

Medians of 5 after two warm-up rounds, with min .. max.   python scripts/safe_ensemble_probe.py"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swimmer_amd as sw  # noqa: E402

DEV = "cuda:0"
REPS, WARM, H, AGENTS, N_DIR = 5, 2, 1000, 20, 8
SIM = (1.02, 0.97, 10.3)
MEMBERS = (1, 8, 64)


def timed_alternately(launches):
    """{label: launch} -> {label: [ms] * REPS}: every repeat runs each launch once, in the given order."""
    ms = {label: [] for label in launches}
    for rep in range(REPS + WARM):
        for label, launch in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            torch.cuda.synchronize()
            if rep >= WARM:
                ms[label].append(e0.elapsed_time(e1))
    return ms


def row(label, ms):
    per = [x / H * 1e6 for x in ms]
    print(f"    {label:<40} ms  median {statistics.median(ms):8.4f}  min {min(ms):8.4f}  max {max(ms):8.4f}   "
          f"ns per step  median {statistics.median(per):7.1f}  ({min(per):.1f} .. {max(per):.1f})", flush=True)
    return statistics.median(per), min(per), max(per)


def members(E):
    """E simulators around SIM, the first SIM itself: distinct constants in the lanes."""
    rs = np.random.RandomState(E)
    rows = np.array(SIM) + np.concatenate([np.zeros((1, 3)), 0.01 * rs.standard_normal((E - 1, 3))])
    return np.tile(rows[None], (AGENTS, 1, 1))


def probe(n):
    A, R = AGENTS, 2 * N_DIR
    p = sw.SwParams.make(n)
    p_lane = sw.SwParams.make(n, flags=sw._lib.FLAG_ROLLOUT_LANE)
    f64 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=DEV)   # noqa: E731
    rs = np.random.RandomState(n)
    policy, deltas = f64(0.1 * (2 * rs.rand(A, p.m, p.d) - 1)), f64(2 * rs.rand(A, N_DIR, p.m, p.d) - 1)
    gated = torch.ones(A, dtype=torch.int32, device=DEV)
    sim_thr, real_thr = f64(np.full(A, np.inf)), f64(np.full(A, 3.0))
    kind, nu = sw._lib.COST_MAX_ABS_THETADOT, 0.03
    i32 = lambda: torch.empty((A, R), dtype=torch.int32, device=DEV)                          # noqa: E731
    # what ARSBatch asks of a launch: returns, the cost maximum, first_refused, violations, status
    out = dict(returns=torch.empty((A, R), dtype=torch.float64, device=DEV),
               cost_max=torch.empty((A, R), dtype=torch.float64, device=DEV), first_refused=i32(), violations=i32(),
               status=i32())
    worst = torch.empty((A, R), dtype=torch.float64, device=DEV)
    mask = torch.empty((A, R), dtype=torch.int64, device=DEV)
    sim1 = f64(np.tile(SIM, (A, 1)))

    def single():
        sw.kernels.safe_ars_rollouts_multi(p_lane, H, policy, deltas, nu, gated, sim1, sim_thr, real_thr, kind, 0, **out)

    def ensemble(E, with_records):
        sims = f64(members(E))
        records = dict(worst_max=worst, refusing_members=mask) if with_records else {}

        def launch():
            sw.kernels.safe_ars_rollouts_ensemble(p, H, policy, deltas, nu, gated, sims, sim_thr, real_thr, kind, 0,
                                                  **out, **records)
        return launch

    launches = {"lane-form kernel, one simulator": single}
    for E in MEMBERS:
        launches[f"ensemble kernel, E = {E:2d}"] = ensemble(E, False)
        launches[f"ensemble kernel, E = {E:2d}, records"] = ensemble(E, True)
    print(f"n = {n}, {A} agents x {R} rollouts x {H} steps, gate open", flush=True)
    ms = timed_alternately(launches)
    print(f"    rollouts that stopped early: {int((out['first_refused'] != H).sum())}, with a status bit: "
          f"{int((out['status'] != 0).sum())}  (both 0: every launch took every step)", flush=True)
    # faster and different is not faster: E = 1 is SIM itself, so at this size too it has the lane-form kernel's bits
    single()
    want = {k: v.clone() for k, v in out.items()}
    launches["ensemble kernel, E =  1"]()
    same = all(torch.equal(v.view(torch.int64) if v.dtype == torch.float64 else v,
                           want[k].view(torch.int64) if v.dtype == torch.float64 else want[k]) for k, v in out.items())
    print(f"    E = 1 against the lane-form kernel, every output bit for bit: {same}", flush=True)
    per = {label: row(label, ms[label]) for label in launches}
    base = per["lane-form kernel, one simulator"][0]
    for with_records in ("", ", records"):
        e1, e8, e64 = (per[f"ensemble kernel, E = {E:2d}{with_records}"] for E in MEMBERS)
        print(f"        E = 1{with_records}: {e1[0] / base:.3f} x the lane-form step;  E = 8 / E = 1: {e8[0] / e1[0]:.3f};  "
              f"E = 64 / E = 1: {e64[0] / e1[0]:.3f}  (repeats of E = 1 spread {e1[2] / e1[1]:.3f}, of E = 64 "
              f"{e64[2] / e64[1]:.3f})", flush=True)


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0), flush=True)
    for n in (3, 6):
        probe(n)
