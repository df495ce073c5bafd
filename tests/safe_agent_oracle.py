"""CPU restatement of the reference's safe ARS iteration (ars/ars_agent.py:137-184 with safe=True), NumPy on the
host with every rollout delegated to the C oracle (oracle/swimmer_oracle.c).

TEST INFRASTRUCTURE ONLY.  For N = 1, and for iterations where all or none of the directions pass, it is the
reference (pinned by tests/test_safe_ars_agent_cpu.py against tests/golden/safe_agent.npz).  With N > 1 and a
partial admission it gives the package's definition where the reference raises IndexError (ars_agent.py:105):
only the k admitted directions are used, each with its own delta, sigma_R over their 2k returns, the step divided
by b.
"""
import numpy as np

from oracle import swimmer_oracle as so


class SafeArsOracle(object):

    def __init__(self, n, real, sim, H, N, b, alpha, nu, V1, threshold, sim_threshold, seed, policy0=None):
        """real / sim: (l_i, m_i, k, h) of the real world and of the simulator."""
        self.p_real = so.OracleParams.make(n, *real)
        self.p_sim = so.OracleParams.make(n, *sim)
        self.m, self.d = n - 1, 2 * n + 2
        self.H, self.N, self.b, self.alpha, self.nu, self.V1 = H, N, b, alpha, nu, V1
        self.threshold, self.sim_threshold = threshold, sim_threshold
        self.policy = np.zeros((self.m, self.d)) if policy0 is None else np.array(policy0, dtype=np.float64)
        self.mean = None if V1 else np.zeros(self.d)
        self.covariance = None if V1 else np.identity(self.d)
        self.saved = []
        self.rng = np.random.RandomState(seed)
        self.violations = 0
        self.last_admitted = np.zeros(0, dtype=np.int64)
        self.db_policies, self.db_trajectories = [], []

    def _sim(self, pol):
        return so.rollout(self.p_sim, self.H, pol, self.mean, self.covariance, want_traj=False)[0]

    def iteration(self):
        deltas = [2 * self.rng.rand(self.m, self.d) - 1 for _ in range(self.N)]
        rewards, admitted = [], []
        for i, dl in enumerate(deltas):
            p1, p2 = self.policy + self.nu * dl, self.policy - self.nu * dl
            if self._sim(p1) <= self.sim_threshold or self._sim(p2) <= self.sim_threshold:
                continue
            admitted.append(i)
            for pol in (p1, p2):
                ret, traj = so.rollout(self.p_real, self.H, pol, self.mean, self.covariance)
                if ret < self.threshold:
                    self.violations += 1
                rewards.append(ret)
                if not self.V1:
                    self.saved.append(traj)
                self.db_policies.append(pol)
                self.db_trajectories.append(traj)
        self.last_admitted = np.array(admitted, dtype=np.int64)
        if rewards:
            r = np.array(rewards).reshape(-1, 2)
            sigma = np.std(r.reshape(-1))
            grad = np.zeros_like(self.policy)
            for j, i in enumerate(admitted):
                grad += (r[j, 0] - r[j, 1]) * deltas[i]
            grad /= self.b * sigma
            self.policy = self.policy + self.alpha * grad
            if not self.V1:
                states = np.concatenate(self.saved, axis=0)
                self.mean = np.mean(states, axis=0)
                self.covariance = np.cov(states.T)
        return rewards

    def training(self, n_iter):
        curve = [np.mean(self.iteration())]          # np.mean([]) = NaN, as in the reference
        for _ in range(n_iter):
            rew = self.iteration()
            curve.append(np.mean(rew) if len(rew) > 0 else curve[-1])
        return np.array(curve)
