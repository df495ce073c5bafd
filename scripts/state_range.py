"""The range of states a trained swimmer visits -- what the reference's ars/state_range.py prints, on this package:
train one V1 agent through Experiment (one seed), load the policy it saved, run one rollout with it and take the
minimum and maximum of every state variable over the rollout.

    python scripts/state_range.py [--iters 300] [--out results/state_range/]

--iters shortens the training (the reference trains 300 iterations); files go under --out."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import swimmer_amd as sw  # noqa: E402

args = argparse.ArgumentParser()
args.add_argument("--iters", type=int, default=300)
args.add_argument("--out", default="results/state_range/")
args = args.parse_args()
out = args.out if args.out.endswith("/") else args.out + "/"
os.makedirs(out, exist_ok=True)

ep = sw.EnvParam("LeonSwimmer", n=3, H=1000, l_i=1., m_i=1., h=1e-3, k=10., epsilon=0)
ap = sw.ARSParam("ARS", V1=True, n_iter=args.iters, H=1000, N=1, b=1, alpha=0.01, nu=0.01, safe=False, threshold=0,
                 initial_w="Zero")
curve = sw.Experiment(ep, results_path=out, save_policy_path=out + "policy").plot(1, ap, plot_mean=False)
print(f"mean return: first iteration {curve[0, 0]}, last {curve[0, -1]}")

total, states = sw.Environment(ep).rollout(np.load(out + "policy.npy"))
states = np.asarray(states)
lo, hi = states.min(axis=0), states.max(axis=0)
print(f"return of one rollout with the trained policy: {total}")
print(f"min per state variable: {lo}")
print(f"max per state variable: {hi}")
names = ["dot(G)_x", "dot(G)_y"] + [f"{q}_{i + 1}" for i in range(ep.n) for q in ("theta", "dot(theta)")]
for name, a, b in zip(names, lo, hi):
    print(f"range of {name}: [{a}, {b}]")
