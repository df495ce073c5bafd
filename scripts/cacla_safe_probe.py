"""What the simulator gate costs CACLA on the swimmer: the gated kernel (sw_cacla_safe_run_f64) beside the plain one
(sw_cacla_run_f64), kernel only, from HIP events around one launch of 4096 steps with the noise already on the device,
in the same process on the same box -- at 1, 64 and 960 agents (one wave each; 960 is the reference's grid), n = 3 and
n = 6 (two hidden units per lane).

Per size four rows: the plain kernel; the gated kernel with every agent ungated (the plain arithmetic behind the
gate's uniform branches); gated with a gate that admits every step (infinite threshold: look-ahead, cost, real step
and update at every step -- the most a step can cost); gated with a gate that refuses every step (NaN threshold: the
forward pass and the look-ahead only).  ns per agent-step = launch time / steps: the agents' waves run side by side.

Medians of 5 after two warm-up launches, with min .. max.   python scripts/cacla_safe_probe.py"""
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
REPS, WARM, STEPS = 5, 2, 4096
SIM = (1.02, 0.97, 10.3)


def timed(launch):
    ms = []
    for rep in range(REPS + WARM):
        fresh = launch(None)                             # clones of the start state, outside the timed region
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(fresh)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms[WARM:]


def row(label, ms):
    per = [x / STEPS * 1e6 for x in ms]
    print(f"    {label:<34} ms  median {statistics.median(ms):8.4f}  min {min(ms):8.4f}  max {max(ms):8.4f}   "
          f"ns per agent-step  median {statistics.median(per):7.1f}  ({min(per):.1f} .. {max(per):.1f})", flush=True)
    return statistics.median(per)


def probe(n, A):
    p = sw.SwParams.make(n)
    f64 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=DEV)   # noqa: E731
    w0 = f64(np.stack([cacla.draw_networks(n, torch.Generator().manual_seed(k)) for k in range(A)]))
    s0 = f64(np.tile(np.array(sw.SwimmerEnv(n=n).reset()), (A, 1)))
    gam, alp = f64(np.full(A, 0.9)), f64(np.full(A, 0.001))
    noise = torch.randn(A, STEPS, n - 1, dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(n))
    rewards = torch.empty(A, STEPS, dtype=torch.float64, device=DEV)
    rec = torch.empty(A, STEPS, dtype=torch.int32, device=DEV)
    sim, real_thr = f64(np.tile(SIM, (A, 1))), f64(np.full(A, 0.05))

    def plain(fresh):
        if fresh is None:
            return w0.clone(), s0.clone()
        sw.kernels.cacla_run(p, STEPS, True, gam, alp, noise, fresh[0], fresh[1], rewards=rewards)

    def gated(flag, thr):
        g = torch.full((A,), flag, dtype=torch.int32, device=DEV)
        sim_thr = f64(np.full(A, thr))

        def launch(fresh):
            if fresh is None:
                return (w0.clone(), s0.clone(), torch.full((A,), float("nan"), dtype=torch.float64, device=DEV),
                        torch.zeros((A, 3), dtype=torch.int32, device=DEV),
                        torch.full((A,), -1, dtype=torch.int32, device=DEV))
            w, s, last, counters, first = fresh
            safe_kernels.cacla_safe_run(p, STEPS, 0, gam, alp, noise, g, sim, sim_thr, real_thr,
                                        sw._lib.COST_MAX_ABS_THETADOT, 0, w, s, last, counters, first,
                                        rewards=rewards, admitted_rec=rec)
        return launch

    print(f"n = {n}, {A} agents x {STEPS} steps", flush=True)
    base = row("plain kernel", timed(plain))
    for label, flag, thr in (("gated kernel, ungated agents", 0, 0.0), ("gated kernel, gate admits all", 1, float("inf")),
                             ("gated kernel, gate refuses all", 1, float("nan"))):
        per = row(label, timed(gated(flag, thr)))
        print(f"        = {per / base:.3f} x the plain step", flush=True)


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0), flush=True)
    for n in (3, 6):
        for A in (1, 64, 960):
            probe(n, A)
