"""CPU restatement of safe_ars/experiment.py's `experience(seed)` (:46-68) and of the costs the script recomputes
(:81-82), on oracle/safe_ars_oracle.py as tests/safe_agent_oracle.py is on the ARS oracle: NumPy on the host, the physics
delegated to the C oracle, one rollout after the other.

TEST INFRASTRUCTURE ONLY.  Pinned by tests/test_safe_experiment_cpu.py against tests/golden/safe_experiment.npz (outputs
of the reference's Basic_ARS.train / Safe_ARS.train, tests/golden/make_safe_experiment_golden.py).
"""
import numpy as np

from oracle import safe_ars_oracle as sao
from oracle import swimmer_oracle as so


def max_abs_thetadot(x):
    return np.max(np.abs(np.asarray(x)[3::2]))                  # experiment.py:44


def basic_rollout(p_real, policy, H):
    """safe_ars/ars.py:20-31.  Returns (R, states [H, d])."""
    obs = so.reset(p_real)
    R, states = 0.0, []
    for _ in range(H):
        obs, rew = so.step(p_real, obs, policy @ obs)
        R += rew
        states.append(obs)
    return R, np.array(states)


def train(p_real, p_sim, gated, cost, real_thresh, sim_thresh, n_iter, N, b, alpha, nu, H, seed):
    """safe_ars/ars.py:67-100 with Basic_ARS.rollout (gated False) or Safe_ARS.rollout.  Returns a dict: curve
    [n_iter], policy, per rollout (n_iter * 2N of them, in the reference's order) its H costs, first refused step and
    real-threshold violations among the steps taken."""
    m, d = p_real.n - 1, 2 * p_real.n + 2
    rng = np.random.RandomState(seed)
    policy = np.zeros((m, d))
    curve, costs, first, viol = [], [], [], []
    for _ in range(n_iter):
        deltas = [2 * rng.rand(m, d) - 1 for _ in range(N)]
        returns = []
        for i in range(N):
            for pol in (policy + nu * deltas[i], policy - nu * deltas[i]):
                if gated:
                    R, states = sao.safe_rollout(p_real, p_sim, cost, sim_thresh, pol, H)
                else:
                    R, states = basic_rollout(p_real, pol, H)
                returns.append(R)
                c = np.array([cost(s) for s in states])
                # a refused rollout repeats its state from the first refused step on; a taken step moves the angles
                reset = so.reset(p_real)
                moved = np.array([not np.array_equal(s, reset if t == 0 else states[t - 1])
                                  for t, s in enumerate(states)])
                taken = int(moved.sum())
                assert moved[:taken].all()
                costs.append(c)
                first.append(taken)
                viol.append(int((c[:taken] > real_thresh).sum()))
        order = np.argsort([max(returns[2 * i], returns[2 * i + 1]) for i in range(N)]).tolist()[::-1][:b]
        used = [returns[2 * i + s] for i in order for s in (0, 1)]
        grad = np.zeros((m, d))
        for i in order:
            grad += (returns[2 * i] - returns[2 * i + 1]) * deltas[i]
        grad /= (len(order) * np.std(used))
        policy = policy + alpha * grad
        curve.append(np.mean(returns))
    return {"curve": np.array(curve), "policy": policy, "costs": np.array(costs),
            "first_refused": np.array(first), "violations": np.array(viol)}


def experience(theta_real, theta_sim, thresh, sim_thresh, n_iter, N, b, alpha, nu, H, seed, n=3, h=1e-3):
    """Both agents of a seed.  theta = (m_i, l_i, k) as the script orders them (:31-39).  Returns (unsafe, safe), each
    train()'s dict plus script_costs: the H costs of the first 2 n_iter rollouts in a row (:81-82)."""
    p_real = so.OracleParams.make(n, theta_real[1], theta_real[0], theta_real[2], h)
    p_sim = so.OracleParams.make(n, theta_sim[1], theta_sim[0], theta_sim[2], h)
    out = []
    for gated in (False, True):
        r = train(p_real, p_sim, gated, max_abs_thetadot, thresh, sim_thresh, n_iter, N, b, alpha, nu, H, seed)
        r["script_costs"] = r["costs"][:2 * n_iter].reshape(-1)
        out.append(r)
    return tuple(out)
