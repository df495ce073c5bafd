"""NumPy restatement of a Safe_ARS rollout gated on an ENSEMBLE of simulators (sw_safe_ars_rollouts_ensemble_f64), on
the C oracle's physics (oracle.swimmer_oracle), one rollout after the other like oracle.safe_ars_oracle.safe_rollout,
whose statements these are with one simulator.

THE ENSEMBLE RULE, stated once (`admits`): at a step every member e looks one step ahead from the real state with the
same action and gives c_e = cost(its next state); the step is taken iff c_e <= sim_thresh for EVERY e (a NaN cost or
threshold refuses).  A refused rollout stops stepping and repeats its state.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import swimmer_oracle as so

MAX, ABS = 1, 0      # SW_COST_MAX_ABS_THETADOT, SW_COST_ABS_OBS


def cost_fn(kind, index):
    """The native costs on an observation [d]: max_i |thetadot_i| (np.max: NaN propagates) or |obs[index]|."""
    if kind == MAX:
        return lambda obs: float(np.max(np.abs(np.asarray(obs)[3::2])))
    return lambda obs: float(abs(np.asarray(obs)[index]))


def admits(member_costs, sim_thresh):
    """The rule: (every member's cost is <= the threshold, the bit mask of the members whose own cost is not)."""
    inside = [bool(c <= sim_thresh) for c in member_costs]
    return all(inside), sum(1 << e for e, ok in enumerate(inside) if not ok)


def rollout(p_real, members, cost, sim_thresh, real_thresh, policy, H, gated=True):
    """One rollout of `policy` [m, d].  members: OracleParams of the ensemble (not read when not gated).  Returns a
    dict: R, states [H, d] (safe_rollout's: the state after step t, the unchanged one where it was refused), costs [H]
    = cost(states[t]), cost_max (0 for H = 0), first_refused (H: none), refusing (the mask at the first refused step,
    0: none), worst_max (the largest member cost over the admitted steps, 0: none admitted, NaN: not gated), violations
    (steps taken with cost > real_thresh) and edge, the smallest |c_e - sim_thresh| over every member cost evaluated."""
    obs = so.reset(p_real)
    R, states, first, refusing, violations, edge = 0.0, [], H, 0, 0, np.inf
    worst = 0.0 if gated else np.nan
    for t in range(H):
        if first < H:                                       # refused: the unchanged state, step after step
            states.append(states[-1] if states else obs)
            continue
        ac = policy @ obs
        if gated:
            member_costs = [cost(so.step(p, obs, ac)[0]) for p in members]
            edge = min(edge, min(abs(c - sim_thresh) for c in member_costs))
            taken, mask = admits(member_costs, sim_thresh)
            if not taken:
                first, refusing = t, mask
                states.append(states[-1] if states else obs)
                continue
            worst = max(worst, max(member_costs))
        obs, rew = so.step(p_real, obs, ac)
        R += rew
        violations += int(cost(obs) > real_thresh)
        states.append(obs)
    states = np.array(states).reshape(H, -1)
    costs = np.array([cost(s) for s in states])
    return dict(R=R, states=states, costs=costs, cost_max=float(np.max(costs)) if H else 0.0, first_refused=first,
                refusing=refusing, worst_max=worst, violations=violations, edge=edge)


def batch(c, H):
    """Every rollout of a case of tests/safe_ensemble_cases.py: a dict of arrays [A, 2 n_dir] (costs: [H, A, 2 n_dir])."""
    n, A, n_dir = c["p"].n, len(c["gated"]), c["deltas"].shape[1]
    p_real = so.OracleParams.make(n, c["p"].l_i, c["p"].m_i, c["p"].k, c["p"].h)
    cost = cost_fn(c["kind"], c["index"])
    keys = ("R", "cost_max", "first_refused", "refusing", "worst_max", "violations", "edge")
    out = {k: np.zeros((A, 2 * n_dir), dtype=np.int64 if k in ("first_refused", "refusing", "violations") else float)
           for k in keys}
    out["costs"] = np.zeros((H, A, 2 * n_dir))
    for a in range(A):
        members = [so.OracleParams.make(n, *row, c["p"].h) for row in c["sims"][a]]
        for r in range(2 * n_dir):
            pol = c["policy"][a] + (-1.0 if r & 1 else 1.0) * c["nu"] * c["deltas"][a, r >> 1]
            one = rollout(p_real, members, cost, c["sim_thresh"][a], c["real_thresh"][a], pol, H, bool(c["gated"][a]))
            for k in keys:
                out[k][a, r] = one[k]
            out["costs"][:, a, r] = one["costs"]
    return out
