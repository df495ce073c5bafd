"""Plain NumPy restatement of ONE CACLA agent on the swimmer behind the simulator gate, for the tests: the loop of the
reference's safe agents (cacla/cacla_safe_agent.py:161-188) with the networks of cacla/cacla_agent.py:165-190
(tests/cacla_oracle.py: forward, update) and the gate of safe_ars/ars.py:111-122.  Initial weights and the noise are
INPUTS, both physics steps are the CPU oracle's (oracle.step_batch).

One step: FA_act = actors(state); action = FA_act + noise[t]; sim_state = the SIMULATOR's step from `state`;
admitted = cost(sim_state) <= sim_thresh (NaN refuses).  Admitted: the real step, violations += cost(new_state) >
real_thresh, temp_diff, critic update, actor update when temp_diff > 0, state = new_state.  Refused: nothing changes.
rewards[t] is the last admitted step's reward, NaN before the first admission (where the reference appends nothing).
"""
import numpy as np

import oracle
from cacla_oracle import forward, update


def abs_obs(index):
    return lambda obs: abs(obs[index])


def max_abs_thetadot(obs):
    return np.max(np.abs(obs[3::2]))          # np.max propagates NaN


def trim(rewards, admitted):
    """The reference's reward list: the entries from the first admitted step on."""
    hit = np.flatnonzero(admitted)
    return list(rewards[hit[0]:]) if hit.size else []


def run(n, gamma, alpha, weights, noise, cost, sim, sim_thresh, real_thresh, gated=True, state0=None,
        l_i=1.0, m_i=1.0, k=10.0, h=1e-3, direction=(1.0, 0.0)):
    """noise [T, n - 1]; sim = (l_i, m_i, k) of the simulator (n, h and direction are the real swimmer's).  Returns a
    dict: rewards [T] (NaN before the first admission), admitted bool [T], counters (admitted, violations,
    actor_updates), first_refused (None if none), weights [n, net_doubles(n)] (a copy, updated), state [d], and the
    run's smallest |cost(sim_state) - sim_thresh| (min_sim_margin), |cost(new_state) - real_thresh| (min_real_margin)
    and |temp_diff| (min_td) -- the distances from the three decisions of a step."""
    p = oracle.OracleParams.make(n, l_i, m_i, k, h, direction)
    p_sim = oracle.OracleParams.make(n, sim[0], sim[1], sim[2], h, direction)
    m = n - 1
    w = np.array(weights, dtype=np.float64, copy=True)
    state = oracle.reset(p) if state0 is None else np.array(state0, dtype=np.float64)
    T = len(noise)
    rewards, admitted = np.full(T, np.nan), np.zeros(T, dtype=bool)
    last = np.nan
    n_adm = n_viol = n_upd = 0
    first_refused = None
    min_sim, min_real, min_td = np.inf, np.inf, np.inf
    for t in range(T):
        fwd = [forward(w[i], state) for i in range(n)]
        fa_act = np.array([f[0] for f in fwd[:m]])
        action = fa_act + noise[t]
        ok = True
        if gated:
            sim_state, _ = oracle.step_batch(p_sim, state[None], action[None])
            c = cost(sim_state[0])
            ok = bool(c <= sim_thresh)
            min_sim = min(min_sim, abs(c - sim_thresh))
        if ok:
            nxt, rew = oracle.step_batch(p, state[None], action[None])
            new_state, reward = nxt[0], float(rew[0])
            c = cost(new_state)
            n_viol += bool(c > real_thresh)
            min_real = min(min_real, abs(c - real_thresh))
            v_new, _, _ = forward(w[m], new_state)
            temp_diff = reward + gamma * v_new - fwd[m][0]
            min_td = min(min_td, abs(temp_diff))
            update(w[m], alpha * temp_diff, state, fwd[m][1], fwd[m][2])
            if temp_diff > 0:
                n_upd += 1
                for i in range(m):
                    update(w[i], alpha * (action[i] - fa_act[i]), state, fwd[i][1], fwd[i][2])
            state = new_state.copy()
            last = reward
            n_adm += 1
            admitted[t] = True
        elif first_refused is None:
            first_refused = t
        rewards[t] = last
    return dict(rewards=rewards, admitted=admitted, counters=(n_adm, n_viol, n_upd), first_refused=first_refused,
                weights=w, state=state, min_sim_margin=min_sim, min_real_margin=min_real, min_td=min_td)
