"""S simulator estimates one after another (Estimator.estimate_real_env_param(method="native")) against ONE
EstimatorBatch.estimate(), on the same box in the same run: S = 1, 8, 80, 320 estimators on the tests/golden/next_rows.npz
store (59-step rollouts, capacity 4) and on a store of 1000-step rollouts (capacity 1), with and without the
least-squares refinement.  Wall-clock medians of --reps runs (default 5) with min..max; the sequential route's search
and refinement are timed apart inside one run each.  Also: the batch's time per generation, and the two kernels' own
times by HIP events (one generation of every estimator; one request for the normal equations of every estimator).
    python scripts/estimator_batch_probe.py [--sizes 1,8,80,320] [--reps 5] [--stores next_rows,h1000]"""
import argparse
import contextlib
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import swimmer_amd as sw
from swimmer_amd import kernels
from swimmer_amd.ars.database import Database
from swimmer_amd.ars.estimator import Estimator
from swimmer_amd.ars.estimator_batch import EstimatorBatch

DEV = "cuda:0"


def next_rows_store():
    g = np.load(os.path.join(ROOT, "tests", "golden", "next_rows.npz"))
    db = Database()
    for P, tr in zip(g["est_policies"], g["est_trajectories"]):
        db.add_trajectory(tr.tolist(), P)
    m_i, l_i, k, h = (float(v) for v in g["est_guess"])
    guess = sw.EnvParam("probe", n=3, H=g["est_trajectories"].shape[1], l_i=l_i, m_i=m_i, h=h, k=k, epsilon=0.0)
    return db, guess, 4


def h1000_store(rollouts=64, H=1000):
    """Rollouts of the reference's real world (l_i 0.8, m_i 1.2, k 10.2) under small random linear policies."""
    rs = np.random.RandomState(3)
    P = 0.2 * (2 * rs.rand(rollouts, 2, 8) - 1)
    p = sw.SwParams.make(3, 0.8, 1.2, 10.2, 1e-3, (1.0, 0.0))
    traj = torch.empty((H, 8, rollouts), dtype=torch.float64, device=DEV)
    kernels.rollout(p, H, torch.as_tensor(P, device=DEV), traj=traj)
    db = Database()
    for r, states in enumerate(traj.permute(2, 0, 1).contiguous().cpu().numpy()):
        db.add_trajectory(states.tolist(), P[r])
    return db, sw.EnvParam("probe", n=3, H=H, l_i=1.0, m_i=1.0, h=1e-3, k=10.0, epsilon=0.0), 1


def spread(ts):
    return f"{np.median(ts) * 1e3:9.1f} ms ({min(ts) * 1e3:.1f}..{max(ts) * 1e3:.1f})"


def sequential(db, guess, capacity, S):
    """-> (search seconds, refinement seconds, generations) of S single estimators, one after another."""
    t_refine, gens = 0.0, []
    t0 = time.perf_counter()
    for a in range(S):
        np.random.seed(a)
        est = Estimator(db, guess, capacity=capacity)
        inner = est._refine

        def timed(x, inner=inner):
            nonlocal t_refine
            t = time.perf_counter()
            out = inner(x)
            t_refine += time.perf_counter() - t
            return out
        est._refine = timed
        with contextlib.redirect_stdout(io.StringIO()):
            est.estimate_real_env_param(method="native", seed=a)
        gens.append(est.generations)
    total = time.perf_counter() - t0
    return total - t_refine, t_refine, gens


def batch(db, guess, capacity, S, refine):
    t0 = time.perf_counter()
    b = EstimatorBatch(db, guess, capacity=capacity, seeds=list(range(S)))
    b.estimate(refine=refine)
    return time.perf_counter() - t0, b


def event_us(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(a.elapsed_time(e) * 1e3)
    return float(np.median(ts))


def kernel_times(b, lam=7):
    """One generation of every estimator (kernel 1) and one normal-equation request of every set (kernel 2, 7 and 1
    points), launches alone, device events."""
    states, nexts, actions, set_begin, lens = b._sets()
    S, longest = b.n_estimators, int(lens.max())
    rng = np.random.default_rng(0)
    X = np.stack([rng.uniform(0.5, 1.5, S * lam), rng.uniform(0.5, 1.5, S * lam), rng.uniform(5, 15, S * lam)], 1)
    order = np.argsort(np.repeat(b.set_of, lam), kind="stable")
    cand = torch.as_tensor(X, device=DEV)
    cand_set = torch.as_tensor(np.repeat(b.set_of, lam)[order].astype(np.int32), device=DEV)
    nb = kernels.step_residual_blocks(longest)
    part = torch.empty((S * lam, nb), dtype=torch.float64, device=DEV)
    val, st = torch.empty(S * lam, dtype=torch.float64, device=DEV), torch.zeros(S * lam, dtype=torch.int32, device=DEV)
    t1 = event_us(lambda: kernels.step_residual_sets(b._base, set_begin, longest, cand, cand_set, states, actions, nexts,
                                                     partial=part, value=val, status=st))
    out = []
    for n_point, K in ((7, 13), (1, 1)):
        pts = torch.as_tensor(np.tile(np.array([0.8, 1.2, 10.2]), (b.n_sets, n_point, 1))
                              * (1 + 1e-6 * rng.standard_normal((b.n_sets, n_point, 3))), device=DEV).contiguous()
        inv = torch.full((b.n_sets, 3), 5e4, dtype=torch.float64, device=DEV) if n_point == 7 else None
        p2 = torch.empty((b.n_sets, K, nb), dtype=torch.float64, device=DEV)
        o2, s2 = torch.empty((b.n_sets, K), dtype=torch.float64, device=DEV), torch.zeros(b.n_sets, dtype=torch.int32,
                                                                                          device=DEV)
        out.append(event_us(lambda: kernels.step_residual_normal_sets(b._base, set_begin, longest, pts, states, actions,
                                                                      nexts, inv_2e=inv, partial=p2, out=o2, status=s2)))
    return t1, out[0], out[1], int(lens.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,80,320")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stores", default="next_rows,h1000")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    print(f"device: {torch.cuda.get_device_name(0)}; medians of {args.reps} (min..max), wall clock")
    for name in args.stores.split(","):
        db, guess, capacity = next_rows_store() if name == "next_rows" else h1000_store()
        batch(db, guess, capacity, 1, True)                       # warm-up: library, allocator, kernels
        for S in sizes:
            seq = [sequential(db, guess, capacity, S) for _ in range(args.reps)]
            bat = {r: [batch(db, guess, capacity, S, r) for _ in range(args.reps)] for r in (False, True)}
            b = bat[True][0][1]
            gens = int(b.generations.max())
            assert list(b.generations) == seq[0][2], "the lock-step searches are the single searches"
            k1, k2n, k2c, T = kernel_times(b)
            ts, tr = [s[0] for s in seq], [s[1] for s in seq]
            tb, tbr = [x[0] for x in bat[False]], [x[0] for x in bat[True]]
            print(f"store {name} (H = {guess.H}, capacity {capacity}), S = {S}: {b.n_sets} sets, {T} transitions, "
                  f"generations {int(b.generations.min())}..{gens} (sum {int(b.generations.sum())})")
            print(f"  sequential  search     {spread(ts)}   + refinement {spread(tr)}")
            print(f"  batch       search     {spread(tb)}   with refinement {spread(tbr)}")
            print(f"  sequential / batch: search {np.median(ts) / np.median(tb):.2f}, with refinement "
                  f"{(np.median(ts) + np.median(tr)) / np.median(tbr):.2f}; batch per generation "
                  f"{np.median(tb) / gens * 1e6:.0f} us ({gens} lock-step generations), per estimator-generation "
                  f"{np.median(tb) / b.generations.sum() * 1e6:.1f} us (sequential {np.median(ts) / b.generations.sum() * 1e6:.1f})")
            print(f"  kernels (HIP events): one generation of all S, lambda 7: {k1:.1f} us; normal equations of all sets "
                  f"(7 points): {k2n:.1f} us; cost (1 point): {k2c:.1f} us", flush=True)


if __name__ == "__main__":
    main()
