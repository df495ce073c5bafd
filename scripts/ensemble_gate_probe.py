"""The ensemble gate against what the library could do without it (n = 3, V1, H = 1000; N = 1 and 8 directions, S = 1 and
80 agents, E = 1 and 8 simulators per agent), one GPU.

    python scripts/ensemble_gate_probe.py [--repeats 5] [--iters 200] [--warmup 10] [--agents 1,80] [--sims 1,8] [--dirs 1,8]

Per case (N, S, E) the inputs are built once; then per repeat, alternating the routes in one process, a host clock
around `iters` calls that end in a device synchronise:
  (a) ars_gate_ensemble: the member launch and the fold, the agents' deltas read in place;
  (b) ars_gate_multi over S * E agents on policy, deltas (and thresholds) replicated E times with
      torch.repeat_interleave, then the torch reductions for admit (amin), worst (NaN to +inf, amin) and status
      (bitwise_or folded over the members) -- the replication and the reductions are inside the timed window: they
      are what the route costs;
  (c) for E = 1 also plain ars_gate_multi over the S agents, which is all a one-member gate needs.
Both routes' admit flags, worst returns and status are compared once per case before timing.
Printed: one JSON line per case and repeat, then per case the median over the repeats with min .. max, microseconds per
call, and whether (a) stays within (b)'s median plus (b)'s own spread."""
import argparse
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
from swimmer_amd import kernels  # noqa: E402
from swimmer_amd.ars.ensemble_kernels import ars_gate_ensemble  # noqa: E402

H, NU, DEV = 1000, 0.01, "cuda:0"
REAL = (0.8, 1.2, 10.2)


def build(N, S, E):
    rng = np.random.RandomState(1000 * N + 10 * S + E)
    f64 = dict(dtype=torch.float64, device=DEV)
    c = dict(policy=torch.tensor(rng.uniform(-0.1, 0.1, (S, 2, 8)), device=DEV),
             deltas=torch.tensor(2 * rng.rand(S, N, 2, 8) - 1, device=DEV),
             sim=torch.tensor(np.array(REAL) + 1e-3 * rng.uniform(-1, 1, (S, E, 3)), device=DEV),
             thr=torch.zeros(S, **f64), p=sw.SwParams.make(3, *REAL, 1e-3, (1.0, 0.0)), N=N, S=S, E=E)
    i32 = dict(dtype=torch.int32, device=DEV)
    c.update(admit=torch.zeros((S, N), **i32), worst=torch.zeros((S, 2 * N), **f64),
             status=torch.zeros((S, 2 * N), **i32), m_ret=torch.zeros((S, E, 2 * N), **f64),
             m_st=torch.zeros((S, E, 2 * N), **i32), m_adm=torch.zeros((S, E, N), **i32),
             b_ret=torch.zeros((S * E, 2 * N), **f64), b_st=torch.zeros((S * E, 2 * N), **i32),
             b_adm=torch.zeros((S * E, N), **i32))
    return c


def route_a(c):
    return ars_gate_ensemble(c["p"], H, c["policy"], c["deltas"], NU, c["sim"], c["thr"], admit=c["admit"],
                             worst=c["worst"], status=c["status"], member_returns=c["m_ret"], member_status=c["m_st"],
                             member_admit=c["m_adm"]) + (c["status"],)


def route_b(c):
    S, E, N = c["S"], c["E"], c["N"]
    kernels.ars_gate_multi(c["p"], H, c["policy"].repeat_interleave(E, dim=0), c["deltas"].repeat_interleave(E, dim=0),
                           NU, c["sim"].view(S * E, 3), c["thr"].repeat_interleave(E), returns=c["b_ret"],
                           status=c["b_st"], admit=c["b_adm"])
    admit = c["b_adm"].view(S, E, N).amin(dim=1)
    r = c["b_ret"].view(S, E, 2 * N)
    worst = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).amin(dim=1)
    st = c["b_st"].view(S, E, 2 * N)
    status = st[:, 0]
    for e in range(1, E):
        status = status | st[:, e]
    return admit, worst, status


def route_c(c):
    return kernels.ars_gate_multi(c["p"], H, c["policy"], c["deltas"], NU, c["sim"].view(c["S"], 3), c["thr"],
                                  returns=c["b_ret"], status=c["b_st"], admit=c["b_adm"])


def timed(route, c, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        route(c)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--agents", default="1,80")
    ap.add_argument("--sims", default="1,8")
    ap.add_argument("--dirs", default="1,8")
    args = ap.parse_args()
    sw._lib.require_gpu()
    torch.cuda.set_stream(torch.cuda.Stream())      # not the null stream
    results = {}
    for N in (int(x) for x in args.dirs.split(",")):
        for S in (int(x) for x in args.agents.split(",")):
            for E in (int(x) for x in args.sims.split(",")):
                c = build(N, S, E)
                routes = {"a_ensemble": route_a, "b_replicated_multi": route_b}
                if E == 1:
                    routes["c_plain_multi"] = route_c
                a, b = [t.clone() for t in route_a(c)], route_b(c)
                torch.cuda.synchronize()
                same = all(torch.equal(x.to(y.dtype), y) for x, y in zip(a, b))
                for route in routes.values():
                    timed(route, c, args.warmup)
                for rep in range(args.repeats):
                    r = dict(N=N, S=S, E=E, repeat=rep, iters=args.iters, routes_agree=bool(same))
                    for name, route in routes.items():
                        r[name + "_us"] = timed(route, c, args.iters)
                    print(json.dumps(r), flush=True)
                    results.setdefault((N, S, E), []).append(r)
    print(f"\nmedian over {args.repeats} repeats (min .. max), microseconds per call (n = 3, V1, H = {H})")
    for (N, S, E), rs in results.items():
        cells, med, spread = [], {}, {}
        for k in [k for k in rs[0] if k.endswith("_us")]:
            v = [r[k] for r in rs]
            med[k], spread[k] = statistics.median(v), max(v) - min(v)
            cells.append(f"{k}={med[k]:.1f} ({min(v):.1f} .. {max(v):.1f})")
        within = med["a_ensemble_us"] <= med["b_replicated_multi_us"] + spread["b_replicated_multi_us"]
        print(f"N={N} S={S} E={E}: " + "  ".join(cells) + f"  a_over_b={med['a_ensemble_us'] / med['b_replicated_multi_us']:.2f}"
              f"  a_within_b_plus_spread={within}  routes_agree={rs[0]['routes_agree']}")


if __name__ == "__main__":
    main()
