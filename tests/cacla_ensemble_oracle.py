"""Plain NumPy restatement of ONE CACLA agent on the swimmer gated on an ENSEMBLE of simulators, for the tests:
tests/cacla_safe_oracle.py::run with the look-ahead in every member.  Initial weights and the noise are INPUTS, all
physics steps are the CPU oracle's (oracle.step_batch).

One step: FA_act = actors(state); action = FA_act + noise[t]; c_e = cost(member e's step from `state`) for every e;
admitted = all(c_e <= sim_thresh) (NaN refuses; a member whose parameters break the library's rule is not stepped and
counts as c_e = +inf).  worst[t] = max_e c_e with NaN -> +inf; member_refusals[e] counts the steps at which member e's
own cost was not <= sim_thresh, whatever the others said.  Admitted / refused: as the single-simulator oracle.
"""
import math

import numpy as np

import oracle
from cacla_oracle import forward, update
from cacla_safe_oracle import abs_obs, max_abs_thetadot, trim  # noqa: F401  (the costs and the list rule, re-exported)


def params_ok(sim):
    """The parameter rule of the library for a member (l_i, m_i, k)."""
    l_i, m_i, k = (float(v) for v in sim)
    return l_i > 0 and m_i > 0 and math.isfinite(l_i) and math.isfinite(m_i) and math.isfinite(k)


def run(n, gamma, alpha, weights, noise, cost, sims, sim_thresh, real_thresh, gated=True, state0=None,
        l_i=1.0, m_i=1.0, k=10.0, h=1e-3, direction=(1.0, 0.0)):
    """noise [T, n - 1]; sims [E][3] = (l_i, m_i, k) of the members (n, h and direction are the real swimmer's).
    Returns what cacla_safe_oracle.run returns -- rewards, admitted, counters, first_refused, weights, state,
    min_real_margin, min_td -- with min_sim_margin the smallest |c_e - sim_thresh| over all members and steps, plus
    worst [T] (NaN when not gated), member_refusals int [E], member_in bool [T, E] (each member's own verdict) and
    bad_member (one breaks the parameter rule: the kernel's SW_STATUS_PARAM)."""
    p = oracle.OracleParams.make(n, l_i, m_i, k, h, direction)
    sims = np.asarray(sims, dtype=np.float64).reshape(-1, 3)
    E = len(sims)
    good = [params_ok(s) for s in sims]
    p_sims = [oracle.OracleParams.make(n, s[0], s[1], s[2], h, direction) if g else None for s, g in zip(sims, good)]
    m = n - 1
    w = np.array(weights, dtype=np.float64, copy=True)
    state = oracle.reset(p) if state0 is None else np.array(state0, dtype=np.float64)
    T = len(noise)
    rewards, admitted = np.full(T, np.nan), np.zeros(T, dtype=bool)
    worst, member_in = np.full(T, np.nan), np.ones((T, E), dtype=bool)
    member_refusals = np.zeros(E, dtype=np.int64)
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
            cs = np.full(E, np.inf)
            for e in range(E):
                if good[e]:
                    sim_state, _ = oracle.step_batch(p_sims[e], state[None], action[None])
                    cs[e] = cost(sim_state[0])
                    min_sim = min(min_sim, abs(cs[e] - sim_thresh))
            with np.errstate(invalid="ignore"):
                member_in[t] = (cs <= sim_thresh) & good             # NaN refuses; a bad member even at sim_thresh = +inf
            member_refusals += ~member_in[t]
            ok = bool(member_in[t].all())
            worst[t] = np.where(np.isnan(cs), np.inf, cs).max()
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
                weights=w, state=state, min_sim_margin=min_sim, min_real_margin=min_real, min_td=min_td,
                worst=worst, member_refusals=member_refusals, member_in=member_in, bad_member=not all(good))
