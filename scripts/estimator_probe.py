"""Cost of one CMA-ES generation of the estimator's objective: ONE population launch (sw_step_residual_pop_f64,
Estimator.I_population's kernel path) against lambda separate I(x) calls (one launch + one .item() each), device
events, median of 20 after warm-up, at T = 19, 236, 65 536 and 1 022 976 stored transitions (n = 3) and lambda = 7, 64.
Also times a full estimate_real_env_param(method="native") on tests/golden/next_rows.npz.
    python scripts/estimator_probe.py"""
import contextlib
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import swimmer_amd as sw
from swimmer_amd import kernels

DEV = "cuda:0"
REPS = 20


def med_us(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main():
    n, d, m = 3, 8, 2
    rng = np.random.default_rng(0)
    print("T, lambda, population launch alone [us], with H2D + D2H [us], lambda x (I launch + .item()) [us], ratio")
    for T in (19, 236, 65536, 1022976):
        s = torch.empty((d, T), dtype=torch.float64, device=DEV)
        s[0:2].uniform_(-0.5, 0.5)
        s[2::2].uniform_(-3, 3)
        s[3::2].uniform_(-2, 2)
        a = torch.empty((m, T), dtype=torch.float64, device=DEV).uniform_(-5, 5)
        nx = s + 1e-3
        base = sw.SwParams.make(n)
        for lam in (7, 64):
            X = np.stack([rng.uniform(0.5, 1.5, lam), rng.uniform(0.5, 1.5, lam), rng.uniform(5, 15, lam)], 1)
            host = torch.as_tensor(X).pin_memory()
            val = torch.zeros(lam, dtype=torch.float64, device=DEV)
            part = torch.empty((lam, kernels.step_residual_blocks(T)), dtype=torch.float64, device=DEV)
            st = torch.zeros(lam, dtype=torch.int32, device=DEV)
            singles = [sw.SwParams.make(n, x[0], x[1], x[2]) for x in X]
            p1 = torch.empty(kernels.step_residual_blocks(T), dtype=torch.float64, device=DEV)

            def pop():
                c = host.to(DEV, non_blocking=True)
                kernels.step_residual_population(base, c, s, a, nx, partial=part, value=val, status=st)
                torch.cat((val, st.to(torch.float64))).cpu()

            def one_by_one():
                for p in singles:
                    kernels.step_residual(p, s, a, nx, partial=p1)
                    float(p1.sum().item())

            dcand = host.to(DEV)

            def launch_only():
                kernels.step_residual_population(base, dcand, s, a, nx, partial=part, value=val, status=st)

            tl, tp, ts = med_us(launch_only), med_us(pop), med_us(one_by_one)
            print(f"{T}, {lam}, {tl:.1f}, {tp:.1f}, {ts:.1f}, {ts / tp:.2f}", flush=True)

    from swimmer_amd.ars.database import Database
    from swimmer_amd.ars.estimator import Estimator
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                             "next_rows.npz"))
    db = Database()
    for P, tr in zip(g["est_policies"], g["est_trajectories"]):
        db.add_trajectory(tr.tolist(), P)
    mi, li, k, h = (float(v) for v in g["est_guess"])
    guess = sw.EnvParam("probe", n=3, H=g["est_trajectories"].shape[1], l_i=li, m_i=mi, h=h, k=k, epsilon=0.0)
    for lam in (None, 16):
        np.random.seed(12)
        est = Estimator(db, guess, capacity=len(g["est_subset"]))
        est.I_population([[mi, li, k]])
        t = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            ep = est.estimate_real_env_param(method="native", seed=0, popsize=lam)
        dt = time.perf_counter() - t
        print(f"estimate_real_env_param(native, lambda={lam or 7}): {dt * 1e3:.1f} ms, {est.generations} generations, "
              f"{dt / est.generations * 1e6:.1f} us/generation, stop {est.stop_reason}, best I {est.best_f:.3e}, "
              f"x = [{ep.m_i:.9f}, {ep.l_i:.9f}, {ep.k:.9f}]")


if __name__ == "__main__":
    main()
