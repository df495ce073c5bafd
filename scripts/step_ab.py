"""Same-box A/B of the step family (csrc/swimmer_step.hip: step, accel, reset, env1 and the four residual entry points)
between two builds of libswimmer_hip.so: are the results the same bits, and is the kernel time the same.

    python scripts/step_ab.py OLD.so NEW.so [--rounds R] [--timeout SECONDS] [--log FILE]

Per round and library two fresh child processes (scripts/ab_common.py has the protocol, the comparison, the noise floor
and the exit codes).  The first child, on the inputs of tests/step_matrix_cases.py at n = 2 .. 8 and both models,

  * saves the outputs of every entry point: step (next state, reward, status), accel and reset at 1, 65, 257 and 513
    environments; the status cases; env1 in both modes on one environment of every regime and on the status cases; the
    single residual at 1, 257 and 1000 transitions; the population at 9 candidates; the sets with SET_OF_CANDIDATE on
    SET_LENGTHS; the normal equations with n_point 1 and 7 and the inactive set; and the NT forms of the residual
    kernels, one launch each per n on the 1024-transition pattern tiled on the device beyond 256 MiB of traffic;
  * times, HIP events around one launch, median of 5 after two warm-up launches, with min and max: sw_step_f64
    through StepPlan at 8192 and 4 194 304 environments, n = 3 and n = 8 (bench.py's aux_step_only);
    sw_step_residual_f64 at 1 022 976 transitions, n = 3 (aux_next_rows' store); the population, sets and
    normal-equations entries at the S = 80 shapes of scripts/estimator_batch_probe.py (both stores; the population:
    the S x 7 candidates on all of a store's transitions).

The second child runs with SWIMMER_STEP_NT=1 (read once per process) and saves the step's outputs again: the NT forms
of step_kernel at test sizes."""
import ctypes
import json
import os
import statistics
import sys

import numpy as np

import ab_common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
REPS, WARM = 5, 2
SIZES = (1, 65, 257, 513)
RES_SIZES = (1, 257, 1000)
POISON = -7.25e77            # never-written entries (rows behind a set's last block, the inactive set) are equal too
S, LAM = 80, 7               # estimator_batch_probe.py: 80 estimators, 7 candidates a generation


def child(out_dir):
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
    import swimmer_amd as sw
    from swimmer_amd import kernels
    import step_matrix_cases as mc

    lib, ptr = sw._lib.load(), sw._lib.ptr
    nt_child = os.environ.get("SWIMMER_STEP_NT") == "1"
    f64 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=DEV)          # noqa: E731
    soa = lambda x: f64(np.asarray(x).T)                                                            # noqa: E731
    i32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=DEV)            # noqa: E731
    poison = lambda *shape: torch.full(shape, POISON, dtype=torch.float64, device=DEV)              # noqa: E731
    arrays = {}

    def keep(name, *tensors):
        for j, t in enumerate(tensors):
            arrays[f"{name}_{j}"] = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.array(t)

    def make(c):
        flags = sw._lib.FLAG_MODEL_TWIN if c["model"] == "twin" else 0
        return sw.SwParams.make(c["n"], c["l"], c["m"], c["k"], c["h"], c["direction"], flags=flags)

    def step(p, st, ac):
        B = st.shape[1]
        out, rew = poison(p.d, B), poison(B)
        sta = torch.full((B,), -77, dtype=torch.int32, device=DEV)
        sw._lib.check(lib.sw_step_f64(ctypes.byref(p), B, ptr(st), ptr(ac), ptr(out), ptr(rew), ptr(sta),
                                      sw._lib.stream_ptr()), "sw_step_f64")
        return out, rew, sta

    # ---- the cases
    for n in mc.NS:
        for model in mc.MODELS[:1] if nt_child else mc.MODELS:      # (the twin model has no NT form)
            c = mc.case(model, n, 0)
            p = make(c)
            batches = [(f"B{B}", c["state"][:B], c["action"][:B]) for B in SIZES]
            batches += [(f"status{kind}",) + mc.status_case(model, n, kind)[:2] for kind in range(len(mc.STATUS_KINDS))]
            for tag, st, ac in batches:
                st, ac = soa(st), soa(ac)
                keep(f"step_{model}_n{n}_{tag}", *step(p, st, ac))
                if not nt_child:
                    keep(f"accel_{model}_n{n}_{tag}", *kernels.accelerations(p, st, ac))
            if nt_child:
                continue
            for B in SIZES:
                keep(f"reset_{model}_n{n}_B{B}", kernels.reset(p, B, device=DEV))
            # env1: one environment of every regime, and lane 0 of every status case
            K, h = kernels.SingleEnv, kernels.SingleEnv()
            pick = [int(np.flatnonzero(c["regime"] == r)[0]) for r in range(len(mc.REGIMES))]
            ones = [(c["state"][e], c["action"][e]) for e in pick]
            ones += [(s[0], a[0]) for s, a, _ in (mc.status_case(model, n, k) for k in range(len(mc.STATUS_KINDS)))]
            got = []
            for st, ac in ones:
                h.io[:] = POISON
                h.io[K.STATE:K.STATE + p.d], h.io[K.ACTION:K.ACTION + n - 1] = st, ac
                status = h.step(p)
                after_step = h.io.copy()
                h.accelerations(p)
                got.append(np.concatenate([after_step, h.io.copy(), [float(status)]]))
            h.close()
            keep(f"env1_{model}_n{n}", np.stack(got))
        if nt_child:
            continue
        # ---- the residual entries (Gym model), on the parameter set the tests use for this n
        pi = n % len(mc.GYM_SETS)
        c, tr = mc.case("gym", n, pi), mc.transitions(n, pi)
        p = make(c)
        cand = f64(mc.candidates(n, pi, mc.POP_CANDIDATES))
        for T in RES_SIZES:
            st, ac, nx = soa(tr["state"][:T]), soa(tr["action"][:T]), soa(tr["stores"]["noise"][:T])
            keep(f"residual_n{n}_T{T}", kernels.step_residual(p, st, ac, nx))
            keep(f"pop_n{n}_T{T}", *kernels.step_residual_population(p, cand, st, ac, nx))
        ts = mc.set_transitions(n, pi)
        st, ac, nx = soa(ts["state"]), soa(ts["action"]), soa(ts["stored"])
        begin = torch.as_tensor(mc.set_begin(), device=DEV)
        longest, n_set = max(mc.SET_LENGTHS), len(mc.SET_LENGTHS)
        nb = kernels.step_residual_blocks(longest)
        cs = i32(mc.SET_OF_CANDIDATE)
        keep(f"sets_n{n}", *kernels.step_residual_sets(p, begin, longest, f64(mc.candidates(n, pi, len(cs))), cs, st,
                                                       ac, nx, partial=poison(len(cs), nb), value=poison(len(cs))))
        for n_point in mc.N_POINTS:
            points, inv = mc.normal_points(n, pi, n_point)
            Kn = 13 if n_point == 7 else 1
            part = poison(n_set, Kn, nb)
            keep(f"normal_n{n}_{n_point}", part, *kernels.step_residual_normal_sets(
                p, begin, longest, f64(points), st, ac, nx, inv_2e=f64(inv) if n_point == 7 else None,
                active=i32(mc.ACTIVE), partial=part, out=poison(n_set, Kn),
                status=torch.full((n_set,), -77, dtype=torch.int32, device=DEV)))
        # the NT forms: the pattern tiled on the device to just beyond kStepStreamBytes
        T = mc.nt_transitions(n)
        q = T // mc.NT_PATTERN
        big = lambda a: torch.cat([soa(a).repeat(1, q), soa(a)[:, :mc.NT_TAIL]], dim=1).contiguous()   # noqa: E731
        st, ac, nx = big(tr["state"]), big(tr["action"]), big(tr["stores"]["noise"])
        assert st.shape[1] == T and T * 8 * (2 * p.d + n) > mc.STREAM_BYTES
        keep(f"residual_nt_n{n}", kernels.step_residual(p, st, ac, nx))
        keep(f"pop_nt_n{n}", *kernels.step_residual_population(p, cand, st, ac, nx))
        del st, ac, nx
        print(f"  cases n = {n}: {len(arrays)} arrays so far", flush=True)
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "cases.npz"), **arrays)
    if nt_child:
        return

    # ---- kernel-only time
    def timed(launch):
        ms = []
        for _ in range(REPS + WARM):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms[WARM:]

    times, rng = {}, np.random.default_rng(0)
    for n in (3, 8):
        p = sw.SwParams.make(n)
        for B in (8192, 1 << 22):
            st = torch.as_tensor(rng.uniform(-1, 1, (p.d, B)), device=DEV)
            ac = torch.as_tensor(rng.uniform(-1, 1, (n - 1, B)), device=DEV)
            out, rew = torch.empty_like(st), torch.empty(B, dtype=torch.float64, device=DEV)
            times[f"sw_step_f64 n={n} {B} envs"] = timed(kernels.StepPlan(p, st, ac, out, rew).launch)
            del st, ac, out, rew
    p, T = sw.SwParams.make(3), 1022976
    st, nx = (torch.as_tensor(rng.uniform(-1, 1, (p.d, T)), device=DEV) for _ in range(2))
    ac = torch.as_tensor(rng.uniform(-1, 1, (2, T)), device=DEV)
    part = torch.empty(kernels.step_residual_blocks(T), dtype=torch.float64, device=DEV)
    times[f"sw_step_residual_f64 n=3 {T} transitions"] = timed(lambda: kernels.step_residual(p, st, ac, nx, partial=part))
    del st, ac, nx

    import estimator_batch_probe as probe
    from swimmer_amd.ars.estimator_batch import EstimatorBatch
    for store in ("next_rows", "h1000"):
        db, guess, capacity = probe.next_rows_store() if store == "next_rows" else probe.h1000_store()
        b = EstimatorBatch(db, guess, capacity=capacity, seeds=list(range(S)))
        states, nexts, actions, set_begin, lens = b._sets()
        longest, total = int(lens.max()), int(lens.sum())
        X = np.stack([rng.uniform(0.5, 1.5, S * LAM), rng.uniform(0.5, 1.5, S * LAM), rng.uniform(5, 15, S * LAM)], 1)
        cand = f64(X)
        cand_set = i32(np.sort(np.repeat(b.set_of, LAM), kind="stable"))
        nb = kernels.step_residual_blocks(longest)
        part, val = poison(S * LAM, nb), poison(S * LAM)
        sta = torch.zeros(S * LAM, dtype=torch.int32, device=DEV)
        shape = f"{store} S={S}: {b.n_sets} sets, {total} transitions"
        times[f"sw_step_residual_sets_f64 {shape}"] = timed(lambda: kernels.step_residual_sets(
            b._base, set_begin, longest, cand, cand_set, states, actions, nexts, partial=part, value=val, status=sta))
        part1 = poison(S * LAM, kernels.step_residual_blocks(total))
        times[f"sw_step_residual_pop_f64 {shape}"] = timed(lambda: kernels.step_residual_population(
            b._base, cand, states, actions, nexts, partial=part1, value=val, status=sta))
        for n_point, Kn in ((7, 13), (1, 1)):
            pts = f64(np.tile(np.array([0.8, 1.2, 10.2]), (b.n_sets, n_point, 1))
                      * (1 + 1e-6 * rng.standard_normal((b.n_sets, n_point, 3))))
            inv = torch.full((b.n_sets, 3), 5e4, dtype=torch.float64, device=DEV) if n_point == 7 else None
            p2, o2 = poison(b.n_sets, Kn, nb), poison(b.n_sets, Kn)
            s2 = torch.zeros(b.n_sets, dtype=torch.int32, device=DEV)
            times[f"sw_step_residual_normal_sets_f64 {n_point} {shape}"] = timed(
                lambda: kernels.step_residual_normal_sets(b._base, set_begin, longest, pts, states, actions, nexts,
                                                          inv_2e=inv, partial=p2, out=o2, status=s2))
    for key, ms in times.items():
        print(f"  {key}: median {statistics.median(ms):.4f} ms", flush=True)
    with open(os.path.join(out_dir, "times.json"), "w") as f:
        json.dump(times, f)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        ab_common.compare(__doc__.split("\n")[0], __file__, children=(("", {}), ("nt_", {"SWIMMER_STEP_NT": "1"})))
