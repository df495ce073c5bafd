"""Rollout launch time and iteration time of the headline ARS V2 iteration (n = 3, capture + V2 moments, full covariance
riding along) in the packed record form ("auto": the lean step with the neighbour's matrix entry, rollout_octs3_kernel;
"lean_v1": the lean step before it, rollout_octl3_kernel; "packed_v1": the first packed kernel, rollout_octp3_kernel)
and the three-store form ("split"), through the native pipeline.  For the loop-placement sweeps of the packed kernels
(SWIMMER_HIP_LIB=... over builds with -DSW_OCTP_LOOP_PAD=k / -DSW_OCTL_LOOP_PAD=k / -DSW_OCTS_LOOP_PAD=k,
scripts/ab_probe.sh) and as a same-process cross-check of the forms.  PK=auto,split chooses the forms (default; a
library from before the lean step knows "auto" and "split" only), PREPS the number of timed blocks of 50 iterations
per form (interleaved).  Design aid."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import swimmer_amd as sw
torch.cuda.set_stream(torch.cuda.Stream("cuda:0"))
N, H = int(os.environ.get('PNDIR', 512)), 1000
forms = os.environ.get('PK', 'auto,split').split(',')
reps = int(os.environ.get('PREPS', 3))
ep = sw.EnvParam("B", n=3, H=H, l_i=1.0, m_i=1.0, h=1e-3, k=10.0, epsilon=0)
ap = sw.ARSParam("B", V1=False, n_iter=0, H=H, N=N, b=N, alpha=0.0075, nu=0.01, safe=False, threshold=0, initial_w="Zero")
agents = {f: sw.ARSAgent(ep, ap, seed=0, device="cuda:0", full_covariance=True, rollout_kernel=f) for f in forms}
kern, wall = {f: [] for f in forms}, {f: [] for f in forms}
for a in agents.values():
    for _ in range(30):
        a.run_iteration_async(want_returns=False)
    torch.cuda.synchronize()
for _ in range(reps):
    for f, a in agents.items():
        a._pipe.timing(1)
        t0 = time.perf_counter()
        for _ in range(50):
            a.run_iteration_async(want_returns=False)
        torch.cuda.synchronize()
        wall[f].append((time.perf_counter() - t0) / 50 * 1e3)
        kern[f].append(a._pipe.rollout_ms()[0])
        a._pipe.timing(0)
print(f"N={N}: " + "; ".join(f"{f} rollout launch {np.median(kern[f]):.4f} (min {min(kern[f]):.4f} max {max(kern[f]):.4f}) "
                             f"iteration {np.median(wall[f]):.4f} ms" for f in forms), flush=True)
