"""Same-box A/B of the three CACLA swimmer kernels (sw_cacla_run_f64, sw_cacla_safe_run_f64,
sw_cacla_safe_ensemble_run_f64) between two builds of libswimmer_hip.so: are the results the same bits, and is the
kernel time the same.

    python scripts/cacla_ab.py OLD.so NEW.so [--rounds R] [--timeout SECONDS] [--log FILE]

Per round and library one fresh child process (scripts/ab_common.py has the protocol, the comparison, the noise
floor and the exit codes).  A child

  * runs fixed-seed cases at n = 2 .. 8, 6 agents x 150 steps (two full 64-step noise blocks and a partial one): the
    plain kernel with train on and off, the gated kernel with gated = [1, 0, 1, 1, 0, 1] behind simulators that
    refuse some steps and admit others (checked), and the ensemble-gated kernel with the same agents behind
    E = 1, 5 and 64 members spread around that simulator (checked likewise), once with the worst-cost record and the
    members' refusal counts and once without either; it saves rewards, weights, state, counters, admit records,
    status, the ensembles and their records to an .npz in a temporary directory;
  * times the kernels alone, HIP events around one launch with the noise already on the device (as
    scripts/cacla_probe.py (c)): the reference's grid of 960 agents at n = 3 x 2048 steps and at n = 8 x 512 steps,
    the gated kernels with every agent gated and a gate that admits every step (look-ahead, real step and update at
    every step), the ensemble-gated one with E = 1 and E = 64 copies of the simulator and both records.  Median of 5
    after two warm-up launches, with min and max.

The parent compares the arrays bit for bit and the timings against the spread of OLD's medians over the rounds."""
import json
import os
import sys

import numpy as np

import ab_common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
REPS, WARM = 5, 2
SIM = (1.02, 0.97, 10.3)
CASE_AGENTS, CASE_STEPS = 6, 150
CASE_GATED = [1, 0, 1, 1, 0, 1]
CASE_MEMBERS, MEMBER_SPREAD = (1, 5, 64), 0.01   # ensemble sizes of the cases; members within 1 % of SIM
TIMED_MEMBERS = (1, 64)
SHAPES = ((3, 2048), (8, 512))          # (n, steps) of the timed launches; 960 agents each


def grid():
    """cacla/swimmer_experiment.py's grid: 10 gammas x 8 alphas x 4 sigmas x 3 seeds = 960 agents."""
    per = [(g, a, s) for g in np.linspace(0.1, 0.95, 10)
           for a in (0.1, 0.03, 0.01, 0.003, 0.001, 0.0003, 0.0001, 0.00003) for s in (1, 0.1, 0.001, 0.0001)
           for _ in range(3)]
    return tuple(np.array([x[i] for x in per], dtype=np.float64) for i in range(3))


def members(A, E):
    """[A, E, 3] simulators for the cases: member 0 is SIM, the others lie within MEMBER_SPREAD of it."""
    spread = np.random.RandomState(E).uniform(-MEMBER_SPREAD, MEMBER_SPREAD, (A, E, 3))
    spread[:, 0] = 0.0
    return np.asarray(SIM) * (1.0 + spread)


def child(out_dir):
    import torch
    sys.path.insert(0, ROOT)
    import swimmer_amd as sw
    from swimmer_amd import cacla
    from swimmer_amd.cacla import safe_kernels

    f64 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=DEV)   # noqa: E731
    i32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=DEV)     # noqa: E731
    max_thetadot = sw._lib.COST_MAX_ABS_THETADOT

    def gate_state(A):
        return (torch.full((A,), float("nan"), dtype=torch.float64, device=DEV),
                torch.zeros((A, 3), dtype=torch.int32, device=DEV), torch.full((A,), -1, dtype=torch.int32, device=DEV))

    # ---- fixed-seed cases
    arrays, A, steps = {}, CASE_AGENTS, CASE_STEPS
    gam, alp = f64(np.linspace(0.5, 0.95, A)), f64([0.01, 0.003] * 3)
    for n in range(2, 9):
        p = sw.SwParams.make(n)
        w0 = f64(np.stack([cacla.draw_networks(n, torch.Generator().manual_seed(40 + a)) for a in range(A)]))
        s0 = f64(np.tile(np.array(sw.SwimmerEnv(n=n).reset()), (A, 1)))
        noise = f64(np.stack([np.random.RandomState(40 + a).normal(0.0, 5.0, (steps, n - 1)) for a in range(A)]))
        for train in (True, False):
            w, s = w0.clone(), s0.clone()
            upd, status = torch.zeros(A, dtype=torch.int32, device=DEV), torch.zeros(A, dtype=torch.int32, device=DEV)
            r = sw.kernels.cacla_run(p, steps, train, gam, alp, noise, w, s, actor_updates=upd, status=status)
            for key, v in (("rewards", r), ("weights", w), ("state", s), ("actor_updates", upd), ("status", status)):
                arrays[f"plain_n{n}_train{int(train)}_{key}"] = v.cpu().numpy()
        w, s, (last, counters, first) = w0.clone(), s0.clone(), gate_state(A)
        rec = torch.empty((A, steps), dtype=torch.int32, device=DEV)
        status = torch.zeros(A, dtype=torch.int32, device=DEV)
        r = safe_kernels.cacla_safe_run(p, steps, 0, gam, alp, noise, i32(CASE_GATED), f64([SIM] * A), f64([0.05] * A),
                                        f64([0.04] * A), max_thetadot, 0, w, s, last, counters, first, admitted_rec=rec,
                                        status=status)
        for key, v in (("rewards", r), ("weights", w), ("state", s), ("last_reward", last), ("counters", counters),
                       ("first_refused", first), ("admitted_rec", rec), ("status", status)):
            arrays[f"gated_n{n}_{key}"] = v.cpu().numpy()
        adm = arrays[f"gated_n{n}_counters"][:, 0]
        print(f"  cases n = {n}: admitted steps per agent {adm.tolist()}, actor updates "
              f"{arrays[f'gated_n{n}_counters'][:, 2].tolist()}", flush=True)
        for a in range(A):
            assert (0 < adm[a] < steps) if CASE_GATED[a] else adm[a] == steps, (n, a, adm[a])
        for E in CASE_MEMBERS:
            sims = members(A, E)
            arrays[f"ens_n{n}_E{E}_sims"] = sims
            for records in (True, False):
                w, s, (last, counters, first) = w0.clone(), s0.clone(), gate_state(A)
                rec = torch.empty((A, steps), dtype=torch.int32, device=DEV)
                status = torch.zeros(A, dtype=torch.int32, device=DEV)
                worst = torch.empty((A, steps), dtype=torch.float64, device=DEV) if records else None
                refusals = torch.zeros((A, E), dtype=torch.int32, device=DEV) if records else None
                r = safe_kernels.cacla_safe_ensemble_run(
                    p, steps, 0, gam, alp, noise, i32(CASE_GATED), f64(sims), f64([0.05] * A), f64([0.04] * A),
                    max_thetadot, 0, w, s, last, counters, first, admitted_rec=rec, worst_rec=worst,
                    member_refusals=refusals, status=status)
                out = [("rewards", r), ("weights", w), ("state", s), ("last_reward", last), ("counters", counters),
                       ("first_refused", first), ("admitted_rec", rec), ("status", status)]
                out += [("worst_rec", worst), ("member_refusals", refusals)] if records else []
                for key, v in out:
                    arrays[f"ens_n{n}_E{E}_records{int(records)}_{key}"] = v.cpu().numpy()
                adm = arrays[f"ens_n{n}_E{E}_records{int(records)}_counters"][:, 0]
                for a in range(A):
                    assert (0 < adm[a] < steps) if CASE_GATED[a] else adm[a] == steps, (n, E, a, adm[a])
            print(f"  cases n = {n}, E = {E}: admitted steps per agent {adm.tolist()}", flush=True)
    np.savez(os.path.join(out_dir, "cases.npz"), **arrays)

    # ---- kernel-only time
    def timed(launch):
        ms = []
        for rep in range(REPS + WARM):
            fresh = launch(None)                         # clones of the start state, outside the timed region
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(fresh)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms[WARM:]

    g, a, sig = grid()
    A, times = len(g), {}
    gam, alp = f64(g), f64(a)
    for n, steps in SHAPES:
        p = sw.SwParams.make(n)
        w0 = f64(np.stack([cacla.draw_networks(n, torch.Generator().manual_seed(k % 3)) for k in range(A)]))
        s0 = f64(np.tile(np.array(sw.SwimmerEnv(n=n).reset()), (A, 1)))
        noise = torch.randn(A, steps, n - 1, dtype=torch.float64, device=DEV,
                            generator=torch.Generator(DEV).manual_seed(n)) * f64(np.sqrt(sig))[:, None, None]
        rewards = torch.empty(A, steps, dtype=torch.float64, device=DEV)
        rec = torch.empty(A, steps, dtype=torch.int32, device=DEV)
        gated, sim = i32(np.ones(A)), f64(np.tile(SIM, (A, 1)))
        sim_thr, real_thr = f64(np.full(A, np.inf)), f64(np.full(A, 0.05))

        def plain(fresh):
            if fresh is None:
                return w0.clone(), s0.clone()
            sw.kernels.cacla_run(p, steps, True, gam, alp, noise, fresh[0], fresh[1], rewards=rewards)

        def gate(fresh):
            if fresh is None:
                return (w0.clone(), s0.clone()) + gate_state(A)
            w, s, last, counters, first = fresh
            safe_kernels.cacla_safe_run(p, steps, 0, gam, alp, noise, gated, sim, sim_thr, real_thr, max_thetadot, 0,
                                        w, s, last, counters, first, rewards=rewards, admitted_rec=rec)

        def ensemble_gate(E):
            sims = f64(np.tile(SIM, (A, E, 1)))
            worst = torch.empty(A, steps, dtype=torch.float64, device=DEV)

            def launch(fresh):
                if fresh is None:
                    refusals = torch.zeros((A, E), dtype=torch.int32, device=DEV)
                    return (w0.clone(), s0.clone()) + gate_state(A) + (refusals,)
                w, s, last, counters, first, refusals = fresh
                safe_kernels.cacla_safe_ensemble_run(p, steps, 0, gam, alp, noise, gated, sims, sim_thr, real_thr,
                                                     max_thetadot, 0, w, s, last, counters, first, rewards=rewards,
                                                     admitted_rec=rec, worst_rec=worst, member_refusals=refusals)
            return launch

        rows = [("sw_cacla_run_f64", plain), ("sw_cacla_safe_run_f64", gate)]
        rows += [(f"sw_cacla_safe_ensemble_run_f64 E={E}", ensemble_gate(E)) for E in TIMED_MEMBERS]
        for name, launch in rows:
            times[f"{name} n={n} {A}x{steps}"] = timed(launch)
    with open(os.path.join(out_dir, "times.json"), "w") as f:
        json.dump(times, f)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        ab_common.compare(__doc__.split("\n")[0], __file__)
