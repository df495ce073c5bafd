"""One safe ARS iteration of S agents: one after another through ARSAgent(safe=True) against one SafeARSAgentBatch
(n = 3, V1, H = 1000, N = 1 and 8 -- the shapes of scripts/safe_ars_probe.py and ars/safe_exploration.py), one GPU.

    python scripts/safe_batch_probe.py [--repeats 5] [--iters 30] [--warmup 5] [--sizes 1,8,80,320] [--dirs 1,8]

Every agent has a simulator of its own (approximate_env_params, epsilon = 1e-3) and a simulator threshold that admits
everything, so every iteration does all of its work: gate, real rollouts, update.  Per case (N, S), agents and batch
are built once; then per repeat, in this order in one process, wall clock around `iters` iterations after a device
synchronise on both sides:
  (a) the S agents one after another, `iters` x runOneIteration() each (a gate launch, the host's read of the admit
      flags, rollouts, update, the host's read of the returns) -- the time of all S agents;
  (b) the batch, `iters` iterations enqueued with run_iteration_async() and ONE read of the history at the end of
      every READ_EVERY iterations, as runTraining() does.
Printed: one JSON line per case and repeat, then per case the median over the repeats with the spread (min .. max), in
microseconds per iteration OF ALL S AGENTS, and the batch's time per agent-iteration."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import swimmer_amd as sw  # noqa: E402
from swimmer_amd.ars.agent_batch import READ_EVERY  # noqa: E402
from swimmer_amd.ars.ars_agent import approximate_env_params  # noqa: E402
from swimmer_amd.ars.parameters import Threshold  # noqa: E402

H = 1000
DB = os.path.join(ROOT, "tests", "golden", "safe_agent_db.npz")


def build(N, S, w0):
    ep = sw.EnvParam("RealWorld", n=3, H=H, l_i=0.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0.001)
    ap = sw.ARSParam("P", V1=True, n_iter=1, H=H, N=N, b=N, alpha=0.0075, nu=0.01, safe=True, threshold=-1e9,
                     initial_w=w0)
    sims = approximate_env_params(ep, 1e-3, S, np.random.RandomState(1))
    agents = []
    with contextlib.redirect_stdout(io.StringIO()):
        for s in range(S):
            agent = sw.ARSAgent(ep, ap, data_path=DB, seed=s, sim_thresh=Threshold(1, 0.3, 0.001),
                                full_covariance=False)
            sim = sims[s]
            agent.estimated_param = sim
            agent.p_sim = sw.SwParams.make(3, sim.l_i, sim.m_i, sim.k, sim.h, (1.0, 0.0))
            agent.sim_threshold = -1e9
            agents.append(agent)
    batch = sw.SafeARSAgentBatch(ep, ap, range(S), sims, [-1e9] * S)
    return agents, batch


def time_agents(agents, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s, agent in enumerate(agents):
        np.random.seed(s)
        for _ in range(iters):
            agent.runOneIteration()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def time_batch(batch, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pending = []
    for j in range(iters):
        pending.append(batch.run_iteration_async())
        if len(pending) == READ_EVERY or j == iters - 1:
            batch._read(pending)
            pending = []
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1,8,80,320")
    ap.add_argument("--dirs", default="1,8")
    args = ap.parse_args()
    torch.cuda.set_stream(torch.cuda.Stream())      # not the null stream (ars_agent.py, Streams)
    w0 = os.path.join(tempfile.mkdtemp(), "w0.npy")
    np.save(w0, np.random.RandomState(7).uniform(-1, 1, (2, 8)))
    results = {}
    quiet = io.StringIO()
    for N in (int(x) for x in args.dirs.split(",")):
        for S in (int(x) for x in args.sizes.split(",")):
            agents, batch = build(N, S, w0)
            with contextlib.redirect_stdout(quiet):
                time_agents(agents, args.warmup)
                time_batch(batch, args.warmup)
                for rep in range(args.repeats):
                    seq, bat = time_agents(agents, args.iters), time_batch(batch, args.iters)
                    r = dict(N=N, S=S, repeat=rep, iters=args.iters, seq_us_per_iter=1e6 * seq / args.iters,
                             batch_us_per_iter=1e6 * bat / args.iters)
                    print(json.dumps(r), file=sys.__stdout__, flush=True)
                    results.setdefault((N, S), []).append(r)
            admitted = sorted({len(a) for a in batch.last_admitted})
            results[(N, S)][-1]["admitted"] = admitted
            del agents, batch
    print(f"\nmedian over {args.repeats} repeats (min .. max), microseconds per iteration of ALL S agents "
          f"(n = 3, V1, H = {H}, everything admitted)")
    for (N, S), rs in results.items():
        cells = []
        for k in ("seq_us_per_iter", "batch_us_per_iter"):
            v = [r[k] for r in rs]
            cells.append(f"{k}={statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})")
        seq = statistics.median(r["seq_us_per_iter"] for r in rs)
        bat = statistics.median(r["batch_us_per_iter"] for r in rs)
        print(f"N={N} S={S}: " + "  ".join(cells) + f"  one_safe_iteration_us={seq / S:.1f}  "
              f"batch_in_single_iterations={bat / (seq / S):.2f}  speedup={seq / bat:.1f}x  "
              f"admitted={rs[-1]['admitted']}")


if __name__ == "__main__":
    main()
