"""The RL-Glue ARS experiment (sw_rlglue_ars_run_f64, one agent per lane, twin model) on one GPU: what a run costs.

  (a) kernel only, from HIP events around the launch with the deltas already on the device: ns per step of the chain
      and per agent-step at A = 1, 64, 960 and 4096 agents, for n = 3 and n = 6 (one wave per workgroup: is the time
      flat in A while the waves have SIMDs to themselves?), at two step counts (is it linear in the steps?);
  (b) end to end, rlglue.SwimmerExperiment at the shipped parameters.txt (n = 3, N = 1, H = 1000) for 100 iterations
      (3 x 10^5 environment steps: the reference's three processes would exchange as many socket round trips), host
      draws, uploads, launches and copies back included; and a batch of 960 such runs.

Medians of 5 after a warm-up, with min .. max.   python scripts/rlglue_probe.py"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swimmer_amd as sw  # noqa: E402
from swimmer_amd import rlglue  # noqa: E402

DEV = "cuda:0"
REPS = 5


def stats(xs):
    return f"median {statistics.median(xs):.4g}  min {min(xs):.4g}  max {max(xs):.4g}"


def kernel_only(n, A, it, N=1, H=100):
    p = sw.SwParams.make(n, h=0.01, flags=sw._lib.FLAG_MODEL_TWIN)
    m, d = p.m, p.d
    deltas = torch.rand(it, N, m, d, A, dtype=torch.float64, device=DEV)
    alpha = torch.full((A,), 0.02, dtype=torch.float64, device=DEV)
    nu = torch.full((A,), 0.02, dtype=torch.float64, device=DEV)
    steps = it * (2 * N + 1) * H
    ms = []
    for rep in range(REPS + 2):
        policy = torch.zeros(m, d, A, dtype=torch.float64, device=DEV)
        carry = torch.zeros(m + 1, A, dtype=torch.float64, device=DEV)
        status = torch.zeros(A, dtype=torch.int32, device=DEV)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sw.kernels.rlglue_ars_run(p, 5.0, 0, it, N, 1, H, alpha, nu, deltas, policy, carry, status)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms[2:])
    print(f"(a) n = {n}  A = {A:5d}  steps = {steps:6d}: ms  {stats(ms[2:])}   {med * 1e6 / steps:8.1f} ns per step of "
          f"the chain, {med * 1e6 / steps / A:9.3f} ns per agent-step   (status {int(status.max())})", flush=True)
    return med


def timed(what, fn):
    out = []
    for rep in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    print(f"{what}: s  {stats(out[1:])}", flush=True)
    return res


def main():
    print(torch.cuda.get_device_name(0), flush=True)
    for n in (3, 6):
        for A in (1, 64, 960, 4096):
            t = [kernel_only(n, A, it) for it in (4, 16)]
            print(f"      steps x 4 -> time x {t[1] / t[0]:.2f}", flush=True)
    ev = timed("(b) SwimmerExperiment, shipped parameters.txt, 100 iterations (3e5 env-steps), end to end",
               lambda: rlglue.SwimmerExperiment(rlglue.Parameters(), seed=0).run(100))
    print("      evaluation returns 0, 49, 99:", ev[0], ev[49], ev[99])
    evs = timed("(b) SwimmerExperimentBatch, 960 seeds of the same, 100 iterations, end to end",
                lambda: rlglue.SwimmerExperimentBatch(rlglue.Parameters(), range(960)).run(100))
    print("      evaluation return 99 over the seeds: min %.6g median %.6g max %.6g" %
          (evs[:, 99].min(), np.median(evs[:, 99]), evs[:, 99].max()))


if __name__ == "__main__":
    main()
