"""Plain NumPy restatement of ONE run of the reference's RL-Glue experiment -- SwimmerARSAgent
(rlglue/agent/SwimmerAgent.py) under the loop of rlglue/experiment/SwimmerExperiment.cpp:65-84 -- for the tests: the
deltas are INPUTS, the physics is the CPU oracle's twin step (oracle.twin_step).

The agent's step counting is unrolled into segments (H environment steps from the saved start state); the arithmetic
is the agent's own, call for call (np.matmul, the two-comparison clip, statistics.stdev, `grad +=`, `grad /=`,
`policy += alpha * grad`), so on one machine it equals the reference bit for bit
(tests/test_rlglue_experiment_cpu.py holds it to tests/golden/rlglue_ars.npz).
"""
from statistics import stdev

import numpy as np

import oracle

START = 0.001          # SwimmerEnvironment.cpp:41


class Run(object):
    """deltas [>= n_it][N][m][d]: sample_deltas() of agent_start, then the one after every iteration.
    perturb: None, or state -> state applied to every new state of the environment (sensitivity runs)."""

    def __init__(self, n, N, b, H, alpha, nu, max_u, deltas, l_i=1.0, m_i=1.0, k=10.0, h=0.01, direction=(1.0, 0.0),
                 perturb=None):
        self.p = oracle.OracleParams.make(n, l_i, m_i, k, h, direction)
        self.n, self.N, self.b, self.H = n, N, b, H
        self.alpha, self.nu, self.max_u = alpha, nu, max_u
        self.m, self.d = n - 1, 2 * n + 2
        self.deltas = np.asarray(deltas, dtype=np.float64)
        self.perturb = perturb
        self.s0 = np.full(self.d, START)
        self.policy = np.zeros((self.m, self.d))
        self.iteration = 0
        self.clips = np.zeros(3, dtype=np.int64)        # components clipped high, clipped low, inside
        self.eval_returns, self.rew, self.policies = [], [], []
        self.stale = self._action(self._pol(0), self.s0)   # agent_start
        self.total = 0.0

    def _pol(self, j):
        delta = self.deltas[self.iteration][j // 2]
        return self.policy + self.nu * delta if j % 2 == 0 else self.policy - self.nu * delta

    def _action(self, policy, state):
        a = np.matmul(policy, np.array(list(state)))
        for i in range(len(a)):
            if a[i] > self.max_u:
                a[i] = self.max_u
                self.clips[0] += 1
            elif a[i] < -self.max_u:
                a[i] = -self.max_u
                self.clips[1] += 1
            else:
                self.clips[2] += 1
        return a.tolist()

    def _segment(self, policy):
        s, a = self.s0, self.stale
        first, rest = 0.0, 0.0
        for t in range(self.H):
            s, r = oracle.twin_step(self.p, s, a)
            if self.perturb is not None:
                s = self.perturb(s)
            if t == 0:
                first = r
                a = self._action(policy, self.s0)
            else:
                rest += r
                a = self._action(policy, s)
        self.stale = a
        return first, rest

    def iterate(self):
        N, b = self.N, self.b
        rew = [0.0] * (2 * N)
        for j in range(2 * N):
            first, rest = self._segment(self._pol(j))
            rew[(j - 1) % (2 * N)] = self.total + first
            self.total = rest
        sigma = stdev(rew[:2 * b])                      # ValueError on a NaN, as in the reference
        grad = np.zeros(self.policy.shape)
        for i in range(b):
            grad += (rew[2 * i] - rew[2 * i + 1]) * self.deltas[self.iteration][i]
        grad /= (b * sigma)
        self.policy += self.alpha * grad
        self.iteration += 1
        first, rest = self._segment(self.policy)        # frozen evaluation
        self.total = rest
        self.rew.append(rew)
        self.policies.append(self.policy.copy())
        self.eval_returns.append(rest)
        return rest

    def run(self, n_it):
        for _ in range(n_it):
            self.iterate()
        return self

    def arrays(self):
        return dict(eval=np.array(self.eval_returns), rew=np.array(self.rew), policies=np.array(self.policies),
                    clips=self.clips.copy())


def relative_noise(seed, scale=1e-13):
    """state -> state * (1 + scale * U(-1, 1)) per component, from a generator of its own."""
    rs = np.random.RandomState(seed)
    return lambda s: s * (1.0 + scale * (2.0 * rs.rand(len(s)) - 1.0))


def sensitivity(make_run, n_it, base, reruns=8, seed0=1000):
    """The largest change of each recorded quantity over `reruns` runs with every new state multiplied by
    1 + 1e-13 U(-1, 1) per component: {eval, rew, policies} -> float."""
    out = dict(eval=0.0, rew=0.0, policies=0.0)
    for r in range(reruns):
        got = make_run(relative_noise(seed0 + r)).run(n_it).arrays()
        for key in out:
            out[key] = max(out[key], float(np.abs(got[key] - base[key]).max()))
    return out
