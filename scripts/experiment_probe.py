"""S seeds of a learning curve trained as one ARSAgentBatch against S ARSAgent trainings one after another
(n = 3, H = 1000), on one GPU.

    python scripts/experiment_probe.py [--repeats 5] [--iters 200] [--warmup 20] [--cases N:S,N:S,...]

Per case (N directions, S seeds, V1 / V2) and per repeat, in this order in one process:
  (a) S x ARSAgent(seed=s, full_covariance=False): `warmup` iterations, then runTraining() over `iters` iterations
      (the host reads the returns every iteration, as the reference's loop does) -- wall time of the S trainings;
  (b) one ARSAgentBatch over the same seeds: the same warm-up, then runTraining() over `iters` iterations (the host
      reads every 10th iteration) -- wall time.
Both clocks stop after a device synchronise.  Then, with HIP events around each launch (median of 50, each queued
behind a rollout launch so that the interval is the device's), the device
time of the rollout launch and of the update launch: one agent's (sw_ars_rollouts_f64 / sw_ars_update_f64) and the
batch's (sw_ars_rollouts_multi_f64 / sw_ars_update_multi_f64).
Printed: one JSON line per case and repeat, then per case the median over the repeats with the spread (min .. max).
Wall times are per iteration OF ALL S SEEDS (for (a): the S trainings' total over `iters`)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import swimmer_amd as sw  # noqa: E402
from swimmer_amd import kernels  # noqa: E402

H = 1000


def params(N, V1, iters):
    ep = sw.EnvParam("LeonSwimmer-RealWorld", n=3, H=H, l_i=.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0)
    ap = sw.ARSParam("Probe", V1=V1, n_iter=iters - 1, H=H, N=N, b=N, alpha=0.0075, nu=0.01, safe=False,
                     threshold=0, initial_w="Zero")
    return ep, ap


def device_us(launch, blocker, reps=50):
    """Median device time of one launch, HIP events around each of `reps` launches.  Each measured launch is queued
    behind `blocker` (a rollout launch of ~0.2 ms): the events and the launch are then in the queue before the device
    reaches them, and the interval is the device's, not the host's enqueue time (the update runs ~5 us)."""
    for _ in range(5):
        launch()
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        blocker()
        e0.record()
        launch()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return 1e3 * statistics.median(a.elapsed_time(b) for a, b in pairs)


def one_case(N, S, V1, iters, warmup):
    ep, ap = params(N, V1, iters)
    quiet = io.StringIO()
    # (a) the seeds one after another
    wall_a = 0.0
    for s in range(S):
        agent = sw.ARSAgent(ep, ap, seed=s, full_covariance=False)
        for _ in range(warmup):
            agent.runOneIteration()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(quiet):
            curve_a = agent.runTraining()
        torch.cuda.synchronize()
        wall_a += time.perf_counter() - t0
    # (b) all seeds at once
    batch = sw.ARSAgentBatch(ep, ap, range(S))
    for _ in range(warmup):
        batch.runOneIteration()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(quiet):
        curve_b = batch.runTraining()
    torch.cuda.synchronize()
    wall_b = time.perf_counter() - t0
    same = bool(np.array_equal(curve_b[S - 1], curve_a))         # the last seed trained alone and in the batch
    # device time of the launches, on the trained state (copies: the timed launches change nothing that is kept)
    p = batch.params
    pol, dl = batch._policy.clone(), batch._deltas.clone()
    mean = None if V1 else batch._mean.clone()
    inv_std = None if V1 else batch._inv_std.clone()
    run = None if V1 else batch._running.clone()
    ret = torch.empty((S, 2 * N), dtype=torch.float64, device=pol.device)
    mom = None if V1 else torch.empty_like(batch._moments)
    n_new = 2 * N * H
    kernels.ars_rollouts_multi(p, H, pol, dl, ap.nu, mean, inv_std, returns=ret, moments=mom)
    one = dict(mean=None if V1 else mean[0], inv_std=None if V1 else inv_std[0], mom=None if V1 else mom[0],
               run=None if V1 else run[0])
    def blocker():
        kernels.ars_rollouts_multi(p, H, pol, dl, ap.nu, mean, inv_std, returns=ret, moments=mom)
    out = {
        "roll_one_us": device_us(lambda: kernels.ars_rollouts(p, H, pol[0], dl[0], ap.nu, 0, N, one["mean"],
                                                              one["inv_std"], returns=ret[0], moments=one["mom"]),
                                 blocker),
        "roll_batch_us": device_us(lambda: kernels.ars_rollouts_multi(p, H, pol, dl, ap.nu, mean, inv_std,
                                                                      returns=ret, moments=mom), blocker),
        "upd_one_us": device_us(lambda: kernels.ars_update(p, ret[0], dl[0], pol[0], 0.0, ap.b, 0, moments=one["mom"],
                                                           running=one["run"], n_new_states=n_new, mean=one["mean"],
                                                           inv_std=one["inv_std"]), blocker),
        "upd_batch_us": device_us(lambda: kernels.ars_update_multi(p, ret, dl, pol, 0.0, ap.b, 0, moments=mom,
                                                                   running=run, n_new_states=n_new, mean=mean,
                                                                   inv_std=inv_std), blocker),
    }
    out.update(N=N, S=S, variant="V1" if V1 else "V2", iters=iters, same_curve=same,
               wall_seq_us_per_iter=1e6 * wall_a / iters, wall_batch_us_per_iter=1e6 * wall_b / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cases", default="1:1,1:8,1:64,8:8")
    args = ap.parse_args()
    cases = [tuple(int(x) for x in c.split(":")) for c in args.cases.split(",")]
    torch.cuda.set_stream(torch.cuda.Stream())      # not the null stream (ars_agent.py, Streams)
    results = {}
    for rep in range(args.repeats):
        for N, S in cases:
            for V1 in (True, False):
                r = one_case(N, S, V1, args.iters, args.warmup)
                r["repeat"] = rep
                print(json.dumps(r), flush=True)
                results.setdefault((N, S, r["variant"]), []).append(r)
    keys = ["wall_seq_us_per_iter", "wall_batch_us_per_iter", "roll_one_us", "roll_batch_us", "upd_one_us",
            "upd_batch_us"]
    print(f"\nmedian over {args.repeats} repeats (min .. max), microseconds; wall = per iteration of all S seeds")
    for (N, S, variant), rs in results.items():
        cells = []
        for k in keys:
            v = [r[k] for r in rs]
            cells.append(f"{k}={statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})")
        print(f"N={N} S={S} {variant} same_curve={all(r['same_curve'] for r in rs)}: " + "  ".join(cells))


if __name__ == "__main__":
    main()
