"""safe_ars/experiment.py both ways on one GPU: all 2 n_seeds agents as one safe_ars.ARSBatch (experiment.run) against
the single-agent route -- per seed Basic_ARS.train, then Safe_ARS.train from the same seed, one agent at a time, every
iteration's [H, d, 2N] trajectory copied to the host (scripts/safe_train_demo.py's loop).

    python scripts/safe_experiment_probe.py [--repeats 5] [--cases fixture,reference] [--launch-iters 200]

Cases: `fixture` (tests/golden/safe_experiment.npz's block a: 2 seeds, N = 4, n_iter = 4, H = 50) and `reference` (the
reference script's own scale: n_seeds = 10, N = 8, b = 4, n_iter = 100, H = 1000, thresh = 3, epsilon = 0.05).  Per case
one untimed warm-up of each route, then per repeat, in this order in one process, wall clock around the whole
experiment after a device synchronise on both sides.  Then the rollout launch of the batch alone, with and without
the cost trace: device events around --launch-iters back-to-back launches, after a warm-up, per repeat.
Printed: one JSON line per measurement, then medians over the repeats with the spread (min .. max)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import swimmer_amd as sw  # noqa: E402
from swimmer_amd.safe_ars import experiment  # noqa: E402

CASES = {
    #            epsilon thresh n_iter H     N  b  alpha nu    n_seeds
    "fixture": (0.5, 1.5, 4, 50, 4, 2, 0.02, 0.5, 2),
    "reference": (0.05, 3.0, 100, 1000, 8, 4, 0.02, 0.03, 10),
}


def setup(case):
    epsilon, thresh, n_iter, H, N, b, alpha, nu, n_seeds = CASES[case]
    u = np.random.RandomState(5).rand(3)
    theta_sim = np.array(experiment.THETA_REAL) + u / np.linalg.norm(u) * epsilon
    return theta_sim, list(range(3, 3 + n_seeds))


def run_batch(case):
    epsilon, thresh, n_iter, H, N, b, alpha, nu, n_seeds = CASES[case]
    theta_sim, seeds = setup(case)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = experiment.run(epsilon, thresh, n_iter, H, N, b, alpha, nu, n_seeds, seeds=seeds, theta_sim=theta_sim)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def run_single(case):
    epsilon, thresh, n_iter, H, N, b, alpha, nu, n_seeds = CASES[case]
    theta_sim, seeds = setup(case)
    tr = experiment.THETA_REAL
    real = sw.SwimmerEnv("RealWorld", n=3, m_i=tr[0], l_i=tr[1], k=tr[2])
    sim = sw.SwimmerEnv("Simulator", n=3, m_i=theta_sim[0], l_i=theta_sim[1], k=theta_sim[2])
    cost = sw.safe_ars.MaxAbsThetaDot()
    curves = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        for seed in seeds:
            for agent in (sw.safe_ars.Basic_ARS(), sw.safe_ars.Safe_ARS(cost, thresh, thresh - 1, sim)):
                np.random.seed(seed)
                curve, states = agent.train(n_iter, real, N, b, alpha, nu, H)
                costs = np.abs(states[:2 * n_iter, :, 3::2]).max(axis=2).reshape(-1)      # experiment.py:81-82
                curves.append((curve, costs))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, curves


def launch_alone(case, iters, with_trace):
    """Milliseconds per rollout launch of the case's batch (zero policies' first iteration: nothing is refused)."""
    epsilon, thresh, n_iter, H, N, b, alpha, nu, n_seeds = CASES[case]
    theta_sim, seeds = setup(case)
    A, dev = 2 * n_seeds, "cuda:0"
    p = sw.SwParams.make(3, 1.0, 1.0, 10.0)
    f64 = dict(dtype=torch.float64, device=dev)
    policy = torch.zeros((A, 2, 8), **f64)
    deltas = torch.as_tensor(2 * np.random.RandomState(1).rand(A, N, 2, 8) - 1, device=dev)
    gated = torch.as_tensor(np.array([0, 1] * n_seeds, dtype=np.int32), device=dev)
    sim = torch.as_tensor(np.tile([theta_sim[1], theta_sim[0], theta_sim[2]], (A, 1)), device=dev)
    sim_thr, real_thr = torch.full((A,), thresh - 1, **f64), torch.full((A,), thresh, **f64)
    ret, cmax = torch.zeros((A, 2 * N), **f64), torch.zeros((A, 2 * N), **f64)
    ints = [torch.zeros((A, 2 * N), dtype=torch.int32, device=dev) for _ in range(3)]
    trace = torch.zeros((H, A, 2 * N), **f64) if with_trace else None

    def go():
        sw.kernels.safe_ars_rollouts_multi(p, H, policy, deltas, nu, gated, sim, sim_thr, real_thr,
                                           sw._lib.COST_MAX_ABS_THETADOT, 0, returns=ret, cost_trace=trace,
                                           cost_max=cmax, first_refused=ints[0], violations=ints[1], status=ints[2])
    for _ in range(10):
        go()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        go()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(values, unit):
    return f"{statistics.median(values):.4g} {unit} ({min(values):.4g} .. {max(values):.4g})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default="fixture,reference")
    ap.add_argument("--launch-iters", type=int, default=200)
    ap.add_argument("--single-repeats", type=int, default=None, help="repeats of the single-agent route (default: --repeats)")
    args = ap.parse_args()
    sw._lib.require_gpu()
    torch.cuda.set_stream(torch.cuda.Stream())
    lines = []
    for case in args.cases.split(","):
        n_single = args.repeats if args.single_repeats is None else args.single_repeats
        _, out = run_batch(case)                       # warm-up, and the agreement of the two routes
        _, curves = run_single(case)
        err = max(float(np.abs(out["unsafe_returns" if a % 2 == 0 else "safe_returns"][a // 2] - c[0]).max())
                  for a, c in enumerate(curves))
        bat, seq = [], []
        for rep in range(args.repeats):
            bat.append(run_batch(case)[0])
            if rep < n_single:
                seq.append(run_single(case)[0])
            print(json.dumps(dict(case=case, repeat=rep, batch_s=bat[-1], single_s=seq[-1] if rep < n_single else None)),
                  flush=True)
        launch = {}
        for with_trace in (False, True):
            launch[with_trace] = [launch_alone(case, args.launch_iters, with_trace) for _ in range(args.repeats)]
            print(json.dumps(dict(case=case, cost_trace=with_trace, launch_ms=launch[with_trace])), flush=True)
        epsilon, thresh, n_iter, H, N, b, alpha, nu, n_seeds = CASES[case]
        lines.append(f"{case}: n_seeds={n_seeds} N={N} b={b} n_iter={n_iter} H={H} thresh={thresh} epsilon={epsilon}\n"
                     f"  whole experiment, batch        : {spread(bat, 's')}\n"
                     f"  whole experiment, single agents: {spread(seq, 's')}   ({len(seq)} repeats)\n"
                     f"  ratio of the medians           : {statistics.median(seq) / statistics.median(bat):.1f}x\n"
                     f"  largest curve difference between the routes: {err:.3g}\n"
                     f"  rollout launch alone, no trace : {spread(launch[False], 'ms')}\n"
                     f"  rollout launch alone, cost trace: {spread(launch[True], 'ms')}")
    print(f"\nmedians over {args.repeats} repeats (min .. max)")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
