"""The training step of the reference's safe-exploration experiment (ars/safe_exploration.py), shortened: a hand
policy from unsafe V1 iterations in the real world, the safety threshold at 99 % of its last mean return, then
ARSAgent(safe=True) with the approximation branch (simulator parameters off by epsilon) from that policy.
Prints the learning curve, how many iterations the simulator gate refused and the violation count.
    HAND=50 ITERS=100 H=1000 EPSILON=0.001 python scripts/safe_ars_demo.py"""
import contextlib
import io
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import swimmer_amd as sw
from swimmer_amd.ars.parameters import Threshold

hand_iters, iters, H = (int(os.environ.get(k, v)) for k, v in (("HAND", 50), ("ITERS", 100), ("H", 1000)))
eps = float(os.environ.get("EPSILON", 0.001))
tmp = tempfile.mkdtemp()
real = dict(n=3, H=H, l_i=0.8, m_i=1.2, h=1e-3, k=10.2, epsilon=eps)          # safe_exploration.py:23-25

hand = sw.ARSAgent(sw.EnvParam("LeonSwimmer-RealWorld", **real),
                   sw.ARSParam("HandControl", V1=True, n_iter=hand_iters - 1, H=H, N=1, b=1, alpha=0.0075, nu=0.01,
                               safe=False, threshold=0, initial_w="Zero"),
                   seed=0, record_trajectories=True)
with contextlib.redirect_stdout(io.StringIO()):
    curve = hand.runTraining(save_data_path=os.path.join(tmp, "real_world.npz"),
                             save_policy_path=os.path.join(tmp, "hand_policy"))
hand.database.save(os.path.join(tmp, "real_world.npz"))
l = curve[-1] * 0.99                                                           # safe_exploration.py:42
print(f"hand policy after {hand_iters} unsafe iterations: mean return {curve[-1]:.6f}; safety threshold {l:.6f}")

np.random.seed(1)
buf = io.StringIO()
with contextlib.redirect_stdout(buf):
    agent = sw.ARSAgent(sw.EnvParam("LeonSwimmer-RealWorld", **real),
                        sw.ARSParam("RLControl", V1=True, n_iter=iters - 1, H=H, N=1, b=1, alpha=0.0075, nu=0.01,
                                    safe=True, threshold=l, initial_w=os.path.join(tmp, "hand_policy.npy")),
                        data_path=os.path.join(tmp, "real_world.npz"), seed=0, approx_error=eps,
                        sim_thresh=Threshold(K=1, A=0.3, B=0.001))
    refused = 0
    inner = agent.runOneIteration

    def counted():
        global refused
        r = inner()
        refused += len(r) == 0
        return r
    agent.runOneIteration = counted
    safe_curve = agent.runTraining()
print(f"simulator threshold {agent.sim_threshold:.6f} (estimated m_i, l_i, k = {agent.estimated_param.m_i:.6f}, "
      f"{agent.estimated_param.l_i:.6f}, {agent.estimated_param.k:.6f})")
print(f"safe training: {iters} iterations, {refused} refused by the simulator gate, "
      f"{agent.violations} real returns below the threshold")
for j in range(0, iters, max(1, iters // 10)):
    print(f"iteration {j:4d}: mean return {safe_curve[j]:.6f}")
print(f"last          : mean return {safe_curve[-1]:.6f}")
