#!/usr/bin/env python3
"""Generate tests/golden/cacla.npz from the reference's own CACLA_agent.run (cacla/cacla_agent.py:135-199) on its own
SwimmerEnv.

Uses the stand-ins of make_golden.py (`gym`, `ray`, `cma` replaced by in-memory modules without arithmetic); the
reference runs unmodified.  Runs only where the reference is available.  Written are DATA only
(numpy.load(allow_pickle=False)); no reference source text is stored.

Cases (seed, n, gamma, alpha, sigma), 256 training steps each after torch.manual_seed(seed); np.random.seed(seed):
  A (0, 3, 0.9, 0.01, 0.1)   B (1, 3, 0.5, 0.1, 1.0)   C (2, 5, 0.95, 0.003, 0.1)   D (3, 2, 0.9, 0.03, 1.0)
  E (4, 8, 0.9, 0.01, 0.1)   and A0: case A with train=False for 64 steps.
Per case: the hyper-parameters, the initial and the final weights (the ActorFA / CriticFA instances the run creates
are recorded through subclasses patched into the module), the noise (a replay of NumPy's stream), the rewards, and
the next np.random.standard_normal() and torch.rand(1) after the run -- witnesses of how much of the two global
streams the run consumed.

Tie condition: a faithful implementation can legitimately differ only where temp_diff or a hidden pre-activation
lies within rounding of 0; every case is asserted to keep |temp_diff| and |z| >= 1e-6 over the whole run.

Usage:  python tests/golden/make_cacla_golden.py
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
_mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mg)          # installs the stand-ins and puts the reference on sys.path

import cacla.cacla_agent as ref  # noqa: E402  (reference module)

MARGIN = 1e-6
# tag: (seed, n, gamma, alpha, sigma, steps, train)
CASES = {
    "A": (0, 3, 0.9, 0.01, 0.1, 256, True),
    "B": (1, 3, 0.5, 0.1, 1.0, 256, True),
    "C": (2, 5, 0.95, 0.003, 0.1, 256, True),
    "D": (3, 2, 0.9, 0.03, 1.0, 256, True),
    "E": (4, 8, 0.9, 0.01, 0.1, 256, True),
    "A0": (0, 3, 0.9, 0.01, 0.1, 64, False),
}


def pack(net):
    """One TwoLayersNet as W1 row-major | b1 | W2 | b2 (the layout of include/swimmer_hip.h)."""
    return np.concatenate([t.detach().numpy().astype(np.float64).reshape(-1)
                           for t in (net.linear1.weight, net.linear1.bias, net.linear2.weight, net.linear2.bias)])


class Recorder(object):
    def __init__(self):
        self.actor = self.critic = None
        self.initial = []
        self.min_td = self.min_z = np.inf

    def saw(self, net, state):
        with torch.no_grad():       # a second look at the pre-activations: reads the weights, draws nothing
            z = net.linear1(torch.tensor(state).double())
        self.min_z = min(self.min_z, float(z.abs().min()))


def run_case(seed, n, gamma, alpha, sigma, steps, train):
    rec = Recorder()

    class ActorFA(ref.ActorFA):
        def __init__(self, *a):
            super().__init__(*a)
            rec.actor = self
            rec.initial += [pack(net) for net in self.network]

        def approximate_action(self, state):
            for net in self.network:
                rec.saw(net, state)
            return super().approximate_action(state)

    class CriticFA(ref.CriticFA):
        def __init__(self, *a):
            super().__init__(*a)
            rec.critic = self
            rec.initial.append(pack(self.network))

        def approximate_value(self, state):
            rec.saw(self.network, state)
            return super().approximate_value(state)

        def update_weigths(self, alpha, delta, state):
            rec.min_td = min(rec.min_td, abs(float(delta)))
            return super().update_weigths(alpha, delta, state)

    keep = ref.ActorFA, ref.CriticFA
    ref.ActorFA, ref.CriticFA = ActorFA, CriticFA
    try:
        torch.manual_seed(seed)
        np.random.seed(seed)
        env = _mg.SwimmerEnv(n=n)
        with contextlib.redirect_stdout(io.StringIO()):
            rewards = ref.CACLA_agent(gamma, alpha, sigma).run(env, steps, train=train)
        next_normal = np.random.standard_normal()
        next_rand = torch.rand(1)
    finally:
        ref.ActorFA, ref.CriticFA = keep
    final = [pack(net) for net in rec.actor.network] + [pack(rec.critic.network)]
    np.random.seed(seed)            # the replay: the run's draws are the first steps * (n - 1) normals of the stream
    noise = np.random.multivariate_normal(np.zeros(n - 1), sigma * np.identity(n - 1), size=steps)
    assert np.random.standard_normal() == next_normal
    assert rec.min_z >= MARGIN and (not train or rec.min_td >= MARGIN), (rec.min_td, rec.min_z)
    return dict(hyper=np.array([seed, n, gamma, alpha, sigma, steps, float(train)]),
                w0=np.stack(rec.initial), w1=np.stack(final), noise=noise,
                rewards=np.array(rewards, dtype=np.float64),
                state=np.array(env.get_state(), dtype=np.float64),
                next_normal=np.float64(next_normal), next_rand=next_rand.numpy().astype(np.float32),
                margins=np.array([rec.min_td, rec.min_z]))


if __name__ == "__main__":
    out = {}
    for tag, case in CASES.items():
        res = run_case(*case)
        print(tag, case, "min |temp_diff| %.3g  min |z| %.3g" % tuple(res["margins"]))
        for k, v in res.items():
            out[f"{tag}_{k}"] = v
    np.savez_compressed(os.path.join(HERE, "cacla.npz"), **out)
    print("wrote", os.path.join(HERE, "cacla.npz"), os.path.getsize(os.path.join(HERE, "cacla.npz")), "bytes")
