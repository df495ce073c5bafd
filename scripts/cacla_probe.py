"""The reference's CACLA grid (cacla/swimmer_experiment.py: 10 gammas x 8 alphas x 4 sigmas x 3 seeds = 960 agents,
n = 3) on one GPU: what a training run costs

  (a) on the fused path, end to end: CACLABatch.run (initial weights and noise drawn on the host, one launch per
      chunk of 2048 steps, one copy of the rewards back), at two chunk counts to see whether the time is linear in
      the steps before anything is scaled to the reference's 10 000;
  (b) the best a user of the package could do WITHOUT the fused kernel: the same 960 agents in lock-step, one
      kernels.step launch per step and batched torch ops on the device for the networks (forward, the lane-local
      backward written as batched tensor ops, masked actor update) -- noise already on the device;
  (c) kernel only, from HIP events around sw_cacla_run_f64 with the noise already on the device: ns and clock cycles
      per agent-step, to set beside the instruction count of the step loop (scripts/isa_loop_stats.py).

Medians of 5 after a warm-up, with min .. max.   python scripts/cacla_probe.py [n_agent_scale]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swimmer_amd as sw  # noqa: E402
from swimmer_amd import cacla  # noqa: E402

DEV = "cuda:0"
N = 3
REPS = 5


def grid():
    gammas = np.linspace(0.1, 0.95, 10)
    alphas = [0.1, 0.03, 0.01, 0.003, 0.001, 0.0003, 0.0001, 0.00003]
    sigmas = [1, 0.1, 0.001, 0.0001]
    per = [(g, a, s) for g in gammas for a in alphas for s in sigmas for _ in range(3)]
    return (np.array([x[0] for x in per]), np.array([x[1] for x in per]), np.array([x[2] for x in per], dtype=float),
            list(range(3)) * (len(per) // 3))


def stats(xs):
    return f"median {statistics.median(xs):.4g}  min {min(xs):.4g}  max {max(xs):.4g}"


def fused_end_to_end(steps):
    g, a, s, seeds = grid()
    env = sw.SwimmerEnv(n=N)
    out = []
    for rep in range(REPS + 1):
        batch = cacla.CACLABatch(env, g, a, s, seeds)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = batch.run(steps)
        out.append(time.perf_counter() - t0)
    print(f"(a) fused, end to end, {len(seeds)} agents x {steps} steps: s  {stats(out[1:])}   "
          f"(finite rewards in {int(np.isfinite(r).all(axis=1).sum())} agents)")
    return statistics.median(out[1:])


def kernel_only(steps):
    g, a, s, seeds = grid()
    A, p = len(seeds), sw.SwParams.make(N)
    w0 = torch.as_tensor(np.stack([cacla.draw_networks(N, torch.Generator().manual_seed(k)) for k in seeds]), device=DEV)
    s0 = torch.as_tensor(np.tile(np.array(sw.SwimmerEnv(n=N).reset()), (A, 1)), device=DEV)
    gam, alp = torch.as_tensor(g, device=DEV), torch.as_tensor(a, device=DEV)
    noise = torch.randn(A, steps, N - 1, dtype=torch.float64, device=DEV) * torch.as_tensor(np.sqrt(s), device=DEV)[:, None, None]
    rewards = torch.empty(A, steps, dtype=torch.float64, device=DEV)
    ms = []
    for rep in range(REPS + 2):
        w, st = w0.clone(), s0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sw.kernels.cacla_run(p, steps, True, gam, alp, noise, w, st, rewards=rewards)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(f"(c) kernel only, {A} agents x {steps} steps: ms  {stats(ms[2:])}")
    return statistics.median(ms[2:])


def lockstep_torch(steps):
    """(b): every array batched over the agents; W1 [A, n, 12, d], b1 / W2 [A, n, 12], b2 [A, n]."""
    g, a, s, seeds = grid()
    A, p, d, m = len(seeds), sw.SwParams.make(N), 2 * N + 2, N - 1
    nets = np.stack([cacla.draw_networks(N, torch.Generator().manual_seed(k)) for k in seeds])
    h = cacla.cacla_agent.HIDDEN
    gam, alp = torch.as_tensor(g, device=DEV), torch.as_tensor(a, device=DEV)
    noise = torch.randn(steps, m, A, dtype=torch.float64, device=DEV) * torch.as_tensor(np.sqrt(s), device=DEV)
    times = []
    for rep in range(REPS + 1):
        W1 = torch.as_tensor(nets[:, :, :h * d].reshape(A, N, h, d), device=DEV).clone()
        b1 = torch.as_tensor(nets[:, :, h * d:h * d + h], device=DEV).clone()
        W2 = torch.as_tensor(nets[:, :, h * d + h:h * d + 2 * h], device=DEV).clone()
        b2 = torch.as_tensor(nets[:, :, -1], device=DEV).clone()
        state = sw.kernels.reset(p, A, DEV)
        nxt, reward = torch.empty_like(state), torch.empty(A, dtype=torch.float64, device=DEV)
        rewards = torch.empty(steps, A, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(steps):
            x = state.t()                                               # [A, d]
            z = torch.einsum("ankd,ad->ank", W1, x) + b1
            hid = torch.relu(z)
            out = (W2 * hid).sum(-1) + b2                               # [A, n]: actors, then V(s)
            action = out[:, :m].t().contiguous() + noise[t]             # [m, A]
            sw.kernels.step(p, state, action, out=nxt, reward=reward)
            zc = torch.einsum("akd,ad->ak", W1[:, m], nxt.t()) + b1[:, m]
            v_new = (W2[:, m] * torch.relu(zc)).sum(-1) + b2[:, m]
            td = reward + gam * v_new - out[:, m]
            step = torch.empty(A, N, dtype=torch.float64, device=DEV)
            step[:, m] = alp * td
            step[:, :m] = torch.where((td > 0)[:, None], alp[:, None] * (action.t() - out[:, :m]), 0.0)
            gpre = torch.where(z > 0, W2, 0.0) * step[:, :, None]       # the old W2
            W2 += step[:, :, None] * hid
            b2 += step
            W1 += gpre[:, :, :, None] * x[:, None, None, :]
            b1 += gpre
            rewards[t] = reward
            state, nxt = nxt, state
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    print(f"(b) lock-step, kernels.step + batched torch ops, {A} agents x {steps} steps: s  {stats(times[1:])}   "
          f"= {statistics.median(times[1:]) / steps * 1e6:.1f} us per step of all agents")
    return statistics.median(times[1:]) / steps


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0))
    k1, k2 = kernel_only(2048), kernel_only(4096)
    A = 960
    per = (k2 - k1) / 2048 * 1e6                                        # ns per step of one agent's wave (all run at once)
    print(f"    kernel: 4096 / 2048 steps = {k2 / k1:.3f}; slope {per:.1f} ns per step, fixed {(2 * k1 - k2) * 1e3:.1f} us; "
          f"at 2.4 GHz {per * 2.4:.0f} cycles per agent-step")
    a1, a2 = fused_end_to_end(2048), fused_end_to_end(4096)
    print(f"    end to end: 4096 / 2048 steps = {a2 / a1:.3f}; slope {(a2 - a1) / 2048 * 1e6:.1f} us per step of all agents, "
          f"fixed {2 * a1 - a2:.3f} s; 10 000 steps: {a1 + (a2 - a1) / 2048 * (10000 - 2048):.2f} s (if linear)")
    b = lockstep_torch(200)
    print(f"    (b) / (a) per step: {b / ((a2 - a1) / 2048):.0f}x on the slope; 10 000 steps of (b): {b * 10000:.1f} s")
