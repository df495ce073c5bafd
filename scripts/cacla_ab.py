"""Same-box A/B of the two CACLA swimmer kernels (sw_cacla_run_f64, sw_cacla_safe_run_f64) between two builds of
libswimmer_hip.so: are the results the same bits, and is the kernel time the same.

    python scripts/cacla_ab.py OLD.so NEW.so [--rounds R] [--timeout SECONDS] [--log FILE]

Per round and library one fresh child process with SWIMMER_HIP_LIB set (OLD, NEW, OLD, NEW, ...), each under its own
time limit; the script stops at the first child that does not exit 0.  A child

  * runs fixed-seed cases at n = 2 .. 8, 6 agents x 150 steps (two full 64-step noise blocks and a partial one): the
    plain kernel with train on and off, and the gated kernel with gated = [1, 0, 1, 1, 0, 1] behind simulators that
    refuse some steps and admit others (checked), and saves rewards, weights, state, counters, admit records and
    status to an .npz in a temporary directory;
  * times the kernels alone, HIP events around one launch with the noise already on the device (as
    scripts/cacla_probe.py (c)): the reference's grid of 960 agents at n = 3 x 2048 steps and at n = 8 x 512 steps,
    the gated kernel with every agent gated and a gate that admits every step (look-ahead, real step and update at
    every step).  Median of 5 after two warm-up launches, with min and max.

The parent compares every array of the two .npz files with np.array_equal (NaNs equal at the same places) and prints
the timings side by side.  With R > 1 the spread of OLD's medians over the rounds is the noise floor: NEW's median
of every round has to lie at or below OLD's largest.  Exit status 1: arrays differ; 3: a time above the floor.

Build OLD in a `git worktree` of the parent commit; a library whose sources are newer than it is rebuilt by the test
suite's conftest (not by this script), so build it last or copy it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
REPS, WARM = 5, 2
SIM = (1.02, 0.97, 10.3)
CASE_AGENTS, CASE_STEPS = 6, 150
CASE_GATED = [1, 0, 1, 1, 0, 1]
SHAPES = ((3, 2048), (8, 512))          # (n, steps) of the timed launches; 960 agents each


def grid():
    """cacla/swimmer_experiment.py's grid: 10 gammas x 8 alphas x 4 sigmas x 3 seeds = 960 agents."""
    per = [(g, a, s) for g in np.linspace(0.1, 0.95, 10)
           for a in (0.1, 0.03, 0.01, 0.003, 0.001, 0.0003, 0.0001, 0.00003) for s in (1, 0.1, 0.001, 0.0001)
           for _ in range(3)]
    return tuple(np.array([x[i] for x in per], dtype=np.float64) for i in range(3))


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

        for name, launch in (("sw_cacla_run_f64", plain), ("sw_cacla_safe_run_f64", gate)):
            times[f"{name} n={n} {A}x{steps}"] = timed(launch)
    with open(os.path.join(out_dir, "times.json"), "w") as f:
        json.dump(times, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per child")
    ap.add_argument("--log", help="also write the report here")
    args = ap.parse_args()
    libs = {"OLD": os.path.abspath(args.old), "NEW": os.path.abspath(args.new)}
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def finish(rc):
        if args.log:
            with open(args.log, "w") as f:
                f.write("\n".join(lines) + "\n")
        sys.exit(rc)

    for tag, path in libs.items():
        if not os.path.exists(path):
            sys.exit(f"{tag}: {path} does not exist")
        say(f"{tag} = {path}")
    medians, differ = {"OLD": {}, "NEW": {}}, 0
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(args.rounds):
            got = {}
            for tag, path in libs.items():
                out = os.path.join(tmp, f"{tag}_{rnd}")
                os.makedirs(out)
                say(f"round {rnd + 1}, {tag}:")
                try:
                    rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out],
                                        env=dict(os.environ, SWIMMER_HIP_LIB=path), timeout=args.timeout).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:
                    say(f"{tag} child ended with status {rc}: stopping here")
                    finish(rc if rc > 0 else 128 - rc)
                with open(os.path.join(out, "times.json")) as f:
                    got[tag] = (dict(np.load(os.path.join(out, "cases.npz"))), json.load(f))
            (a_old, t_old), (a_new, t_new) = got["OLD"], got["NEW"]
            bad = [k for k in a_old if k not in a_new or not np.array_equal(a_old[k], a_new[k],
                                                                            equal_nan=a_old[k].dtype.kind == "f")]
            bad += [k for k in a_new if k not in a_old]
            differ += len(bad)
            say(f"round {rnd + 1}: {len(a_old) - len(bad)} of {len(a_old)} arrays bit-equal"
                + ("" if not bad else "; DIFFERENT: " + ", ".join(bad)))
            for key in t_old:
                o, n = t_old[key], t_new[key]
                medians["OLD"].setdefault(key, []).append(statistics.median(o))
                medians["NEW"].setdefault(key, []).append(statistics.median(n))
                say(f"  {key:<42} ms  OLD median {statistics.median(o):8.4f} ({min(o):.4f} .. {max(o):.4f})   "
                    f"NEW median {statistics.median(n):8.4f} ({min(n):.4f} .. {max(n):.4f})   "
                    f"NEW / OLD {statistics.median(n) / statistics.median(o):.4f}")
    above = 0
    if args.rounds > 1:
        say("over the rounds (ms): OLD's medians min .. max are the noise floor; NEW's medians must not exceed "
            "OLD's max")
        for key, o in medians["OLD"].items():
            n = medians["NEW"][key]
            ok = max(n) <= max(o)
            above += 0 if ok else 1
            say(f"  {key:<42} OLD {min(o):8.4f} .. {max(o):8.4f}   NEW {min(n):8.4f} .. {max(n):8.4f}   "
                + ("at or below" if ok else "ABOVE"))
    say("arrays: " + ("all bit-equal" if not differ else f"{differ} DIFFERENT"))
    finish(1 if differ else 3 if above else 0)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
