"""Cost of a safe ARS iteration (ARSAgent(safe=True)) next to an unsafe one, device events after warm-up.

Shapes: the reference's experiment (n = 3, V1, N = 1, H = 1000, ars/safe_exploration.py) and n = 3, V2, N = 512,
H = 1000 with the simulator threshold at the median of the simulator returns around the start policy (the policy
moves during the timed iterations, so the admitted count of the last one is printed next to the time).  Also times
the gate launch alone against the plain rollout launch (ars_rollouts without trajectories) at the same n and N.  Run it once under `rocprofv3 --kernel-trace --stats` in a run of its own for
the kernels' own durations (ars_gate_oct3_kernel vs rollout_oct3_kernel).
    python scripts/safe_ars_probe.py [--quick] [--only N]      (--only: just the shape with N directions)"""
import contextlib
import io
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import swimmer_amd as sw
from swimmer_amd import kernels
from swimmer_amd.ars.parameters import Threshold

QUICK = "--quick" in sys.argv
REPS = 5 if QUICK else 20
DB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                  "safe_agent_db.npz")


def ms(fn, reps=REPS):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def agents(V1, N, H):
    tmp = tempfile.mkdtemp()
    w0 = os.path.join(tmp, "w0.npy")
    np.save(w0, np.random.RandomState(7).uniform(-1, 1, (2, 8)))
    out = []
    for safe in (True, False):
        ep = sw.EnvParam("RealWorld", n=3, H=H, l_i=0.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0.001)
        ap = sw.ARSParam("P", V1=V1, n_iter=1, H=H, N=N, b=N, alpha=0.0075, nu=0.1, safe=safe,
                         threshold=-1e9, initial_w=w0)
        kw = dict(data_path=DB, sim_thresh=Threshold(1, 0.3, 0.001)) if safe else {}
        with contextlib.redirect_stdout(io.StringIO()):
            out.append(sw.ARSAgent(ep, ap, seed=1, **kw))
    return out


def main():
    H = 1000
    only = int(sys.argv[sys.argv.index("--only") + 1]) if "--only" in sys.argv else None
    for V1, N in ((True, 1), (False, 512)):
        if only is not None and N != only:
            continue
        safe, plain = agents(V1, N, H)
        if N > 1:       # about half admitted: the median of the simulator returns around the start policy
            st = np.random.get_state()
            d = torch.tensor(2 * np.random.rand(N, 2, 8) - 1, device="cuda:0")
            np.random.set_state(st)
            r = kernels.ars_rollouts(safe.p_sim, H, safe._policy, d, 0.1, 0, N).cpu().numpy()
            safe.sim_threshold = float(np.median(np.minimum(r[0::2], r[1::2])))
        t_safe = ms(lambda: safe.runOneIteration())
        t_plain = ms(lambda: plain.runOneIteration())
        k = len(safe.last_admitted)
        d = torch.tensor(2 * np.random.rand(N, 2, 8) - 1, device="cuda:0")
        mean, inv = (None, None) if V1 else (safe._mean, safe._inv_std)
        t_gate = ms(lambda: kernels.ars_gate(safe.p_sim, H, safe._policy, d, 0.1, 0, N, 0.0, mean=mean,
                                             inv_std=inv))
        t_roll = ms(lambda: kernels.ars_rollouts(safe.p_sim, H, safe._policy, d, 0.1, 0, N, mean=mean,
                                                 inv_std=inv))
        tag = f"n=3 {'V1' if V1 else 'V2'} N={N} H={H}"
        print(f"{tag}: safe iteration {t_safe:.4f} ms (last admitted {k}/{N}), unsafe iteration {t_plain:.4f} ms")
        print(f"{tag}: gate launch {t_gate:.4f} ms, plain rollout launch (no trajectories) {t_roll:.4f} ms; "
              f"gate/rollout = {t_gate / t_roll:.3f}" + ("" if t_gate <= t_roll else
                                                          f" (gate slower by {100 * (t_gate / t_roll - 1):.1f} %)"))


if __name__ == "__main__":
    main()
