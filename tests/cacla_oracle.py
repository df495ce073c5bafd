"""Plain NumPy restatement of ONE CACLA agent on the swimmer (the reference's cacla/cacla_agent.py:135-199 with
TwoLayersNet / ActorFA / CriticFA, :19-132), for the tests: initial weights and the noise are INPUTS, the physics is
the CPU oracle's (oracle.step_batch).

Networks are vectors in the layout of include/swimmer_hip.h: W1 [12][d] row-major | b1 [12] | W2 [12] | b2; an agent
is its n - 1 actors followed by the critic.  The backward pass of update_weights is written out: with z = W1 x + b1,
h = relu(z) from the forward at the same state, g = (z > 0) * W2 (the old W2), and
W2 += step h, b2 += step, W1 += step outer(g, x), b1 += step g.
"""
import numpy as np

import oracle

HIDDEN = 12


def net_doubles(n):
    return HIDDEN * (2 * n + 2) + 2 * HIDDEN + 1


def views(vec, d):
    """(W1 [12, d], b1 [12], W2 [12], b2 [1]) as views into one network's vector."""
    a, b = HIDDEN * d, HIDDEN * d + HIDDEN
    return vec[:a].reshape(HIDDEN, d), vec[a:b], vec[b:b + HIDDEN], vec[b + HIDDEN:b + HIDDEN + 1]


def forward(vec, x):
    w1, b1, w2, b2 = views(vec, x.shape[0])
    z = w1 @ x + b1
    h = np.where(z > 0, z, 0.0)
    return float(w2 @ h + b2[0]), z, h


def update(vec, step, x, z, h):
    w1, b1, w2, b2 = views(vec, x.shape[0])
    g = np.where(z > 0, w2, 0.0)
    w2 += step * h
    b2 += step
    w1 += step * np.outer(g, x)
    b1 += step * g


def run(n, gamma, alpha, weights, noise, state0=None, train=True, l_i=1.0, m_i=1.0, k=10.0, h=1e-3,
        direction=(1.0, 0.0)):
    """noise [T, n - 1] is added to the actors' outputs.  Returns a dict: rewards [T], weights [n, net_doubles(n)]
    (a copy, updated), state [d] (the swimmer's), actor_updates, and the run's smallest |temp_diff| and |z|
    (the distances from the two discontinuities of a step)."""
    p = oracle.OracleParams.make(n, l_i, m_i, k, h, direction)
    m = n - 1
    w = np.array(weights, dtype=np.float64, copy=True)
    env_state = oracle.reset(p) if state0 is None else np.array(state0, dtype=np.float64)
    state = env_state.copy()
    T = len(noise)
    rewards = np.empty(T)
    n_upd, min_td, min_z = 0, np.inf, np.inf
    for t in range(T):
        fwd = [forward(w[i], state) for i in range(n)]
        fa_act = np.array([f[0] for f in fwd[:m]])
        action = fa_act + noise[t]
        nxt, rew = oracle.step_batch(p, env_state[None], action[None])
        env_state, reward = nxt[0], float(rew[0])
        rewards[t] = reward
        min_z = min(min_z, min(np.abs(f[1]).min() for f in fwd))
        if train:
            v_new, z_new, _ = forward(w[m], env_state)
            temp_diff = reward + gamma * v_new - fwd[m][0]
            min_td, min_z = min(min_td, abs(temp_diff)), min(min_z, np.abs(z_new).min())
            update(w[m], alpha * temp_diff, state, fwd[m][1], fwd[m][2])
            if temp_diff > 0:
                n_upd += 1
                for i in range(m):
                    update(w[i], alpha * (action[i] - fa_act[i]), state, fwd[i][1], fwd[i][2])
            state = env_state.copy()
    return dict(rewards=rewards, weights=w, state=env_state, actor_updates=n_upd, min_td=min_td, min_z=min_z)
