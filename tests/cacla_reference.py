"""A long-double reference for ONE step of the CACLA swimmer kernels (csrc/swimmer_cacla_learner.h with
swimmer_cacla.hip, swimmer_cacla_safe.hip and swimmer_cacla_ensemble.hip), and the bounds the kernels are held to.
Nothing here touches the GPU.

THE REFERENCE restates one step of cacla_agent.py:170-193 in np.longdouble (64-bit significand) in the layout of
include/swimmer_hip.h (a network is W1 [12][d] | b1 [12] | W2 [12] | b2, an agent its n - 1 actors and then the
critic), the gated step of sw_cacla_safe_run_f64 and the ensemble gate of sw_cacla_safe_ensemble_run_f64.  The physics
is tests/step_reference.py's (accelerations_ld, euler, step_ref: the Gym model), not restated.

THE BOUNDS.  Next to every long-double value runs a float64 first-order bound on what a correct fp64 evaluation may
differ by: u = 2^-53, gamma_j of step_reference; the roundings of each stage are counted off swimmer_cacla_learner.h,
and an input's error passes on through the stage's absolute partial derivatives.

 * unit_input   z = W1[j, :] . x + b1[j]: two fma chains of D / 2 roundings each and one add:
                gamma_(D/2 + 1) (|b1| + sum |w x|) + sum |w| e_x                       (e_x = 0 at the old state)
 * relu         h = z or 0, e_h = e_z or 0 -- the decision z <= 0 is a MARGIN of the case, not part of the bound
 * output       p_j = W2_j h_j (one rounding), sum_hidden's four levels, then + b2:
                sum (|W2_j| e_h + u |p_j|) + gamma_5 (sum |p_j| + |b2|)
 * action       out + noise: e_out + u |action|
 * physics      step_ref's bound at the reference action with the project's K = 32 for the Gym model, plus
                sum_i |d step / d u_i| e_action_i, the sensitivities by central differences in long double (step 2^-26
                relative to max(1, |u_i|); the step is affine in the torques)
 * td           (reward + gamma V(s')) - V(s), three roundings:
                e_r + |gamma| e_V' + e_V + u (|gamma V'| + |reward + gamma V'| + |td|)
 * st           alpha td: |alpha| e_td + u |st|; an actor's alpha (action - FA_act): two roundings
 * weights      sg = st W2 (one multiply), then one fma or one add per entry:
                W2' = fma(st, h, W2): |h| e_st + |st| e_h + u |W2'|;   W1' = fma(sg, x, W1): |x| e_sg + u |W1'|
                b1' = b1 + sg: e_sg + u |b1'|;                          b2' = b2 + st: e_st + u |b2'|
                A unit that is off has sg = 0 and h = 0 exactly: its W1 row, b1 and W2 keep their bits (bound 0), and
                so does every entry of a network that takes no update.
 * costs        |obs[i]|: the entry's bound; max_i |thetadot_i|: the largest of the entries' bounds.

The long-double arithmetic's own roundings (2^-64 each) are 2^-11 of the fp64 ones and are not carried.  A kernel's
tolerance is K times the running bound, K measured on the float64 NumPy oracles (tests/cacla_matrix_cases.py).
A ratio above K is a failure, never a reason for a larger K.

MUTANTS (tests/test_cacla_matrix_cpu.py: the bound must show each): 1 the gradient uses the updated W2; 2 V(s') is
taken after the critic's update (the critic is stepped by the right td, V(s') read from the stepped weights, and the
td formed from it is the one the original weights are stepped by); 3 the actors update whatever the sign of td; 4 b2
is not updated; 5 the gradient's x is the new state; 6 the actor's step is alpha action.
"""
import numpy as np

import step_reference as sr
from step_reference import LD, U, Ref, gamma

HIDDEN = 12
K_GYM = 32.0                       # the step matrix's K for the Gym model (tests/step_matrix_cases.py)
COST_ABS_OBS, COST_MAX_ABS_THETADOT = 0, 1


def net_doubles(n):
    return HIDDEN * (2 * n + 2) + 2 * HIDDEN + 1


def views(vec, d):
    a, b = HIDDEN * d, HIDDEN * d + HIDDEN
    return vec[:a].reshape(HIDDEN, d), vec[a:b], vec[b:b + HIDDEN], vec[b + HIDDEN]


def _ld(x):
    return LD(1) * np.asarray(x, dtype=np.float64)


def _abs(x):
    return np.abs(x).astype(np.float64)


def hidden(vec, x):
    """Ref [12]: z of one network (float64 vector) at the observation x (Ref [d])."""
    d = x.value.shape[0]
    w1, b1, _, _ = views(_ld(vec), d)
    z = w1 @ x.value + b1
    mag = _abs(b1) + _abs(w1) @ _abs(x.value)
    return Ref(z, gamma(d // 2 + 1) * mag + _abs(w1) @ x.bound)


def output(vec, z):
    """(Ref scalar: the network's output, Ref [12]: h, bool [12]: the units that are on)."""
    d = (len(vec) - 2 * HIDDEN - 1) // HIDDEN
    _, _, w2, b2 = views(_ld(vec), d)
    on = z.value > 0
    h = Ref(np.where(on, z.value, LD(0)), np.where(on, z.bound, 0.0))
    p = w2 * h.value
    ep = _abs(w2) * h.bound + U * _abs(p)
    out = p.sum() + b2
    return Ref(out, float(ep.sum() + gamma(5) * (_abs(p).sum() + abs(float(b2))))), h, on


def forward(n, w, state, noise):
    """The actors' and the critic's forward at `state` and the action: dict(x, z [n], out [n], h [n], on [n],
    action Ref [n - 1])."""
    x = Ref(_ld(state), np.zeros(2 * n + 2))
    z = [hidden(w[i], x) for i in range(n)]
    res = [output(w[i], z[i]) for i in range(n)]
    fa = np.array([r[0].value for r in res[:n - 1]], dtype=LD)
    efa = np.array([r[0].bound for r in res[:n - 1]])
    act = fa + _ld(noise)
    return dict(x=x, z=z, out=[r[0] for r in res], h=[r[1] for r in res], on=[r[2] for r in res],
                action=Ref(act, efa + U * _abs(act)))


def physics(rows, h, direction, state, action):
    """The Gym model's step from `state` (exact doubles [d]) with `action` (Ref [n - 1]) for every row (l, m, k) of
    rows [E, 3]: (Ref next [E, d], Ref reward [E])."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    E = len(rows)
    l, m, k = rows[:, 0], rows[:, 1], rows[:, 2]
    st = np.tile(np.asarray(state, dtype=np.float64), (E, 1))
    a64 = np.tile(action.value.astype(np.float64), (E, 1))
    at = sr.step_ref("gym", l, m, k, h, direction, st, a64, K=K_GYM)
    n, Gd, s, c, thd, _ = sr.unpack(st, a64)

    def f(u):
        return sr.euler("gym", h, direction, st, sr.accelerations_ld(n, l, m, k, Gd, s, c, thd, u))
    u = np.tile(action.value, (E, 1))
    nxt, rew = f(u)
    en, er = at["next"].bound.copy(), at["reward"].bound.copy()
    for i in range(n - 1):
        dlt = sr.EPS * max(LD(1), abs(action.value[i]))
        up, um = u.copy(), u.copy()
        up[:, i] += dlt
        um[:, i] -= dlt
        (np_, rp), (nm, rm) = f(up), f(um)
        en += (np.abs(np_ - nm) / (2 * dlt)).astype(np.float64) * action.bound[i]
        er += (np.abs(rp - rm) / (2 * dlt)).astype(np.float64) * action.bound[i]
    return Ref(nxt, en), Ref(rew, er)


def cost(obs, kind, index):
    """Ref of the cost of states obs (Ref [..., d])."""
    if kind == COST_ABS_OBS:
        return Ref(np.abs(obs.value[..., index]), obs.bound[..., index])
    return Ref(np.abs(obs.value[..., 3::2]).max(axis=-1), obs.bound[..., 3::2].max(axis=-1))


def _updated(vec, st, x, h, on, mutant):
    """Ref [NETD]: the network after update_weights with step st (Ref scalar) at x (LD [d]; h, on from its forward)."""
    d = x.shape[0]
    w1, b1, w2, b2 = views(_ld(vec), d)
    sv, sb = st.value, st.bound
    w2n = w2 + sv * h.value
    g = np.where(on, w2n if mutant == 1 else w2, LD(0))
    sg = sv * g
    esg = _abs(g) * sb + U * _abs(sg)
    w1n = w1 + sg[:, None] * x[None, :]
    b1n = b1 + sg
    b2n = b2 if mutant == 4 else b2 + sv
    ew1 = np.where(on[:, None], _abs(x)[None, :] * esg[:, None] + U * _abs(w1n), 0.0)
    eb1 = np.where(on, esg + U * _abs(b1n), 0.0)
    ew2 = np.where(on, _abs(h.value) * sb + abs(float(sv)) * h.bound + U * _abs(w2n), 0.0)
    eb2 = sb + U * abs(float(b2n))
    return Ref(np.concatenate([w1n.ravel(), b1n, w2n, [b2n]]), np.concatenate([ew1.ravel(), eb1, ew2, [eb2]]))


def _edge(value, bound):
    """The smallest |value| / bound: how many bounds a decision lies from its edge."""
    value, bound = _abs(np.atleast_1d(value)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    with np.errstate(divide="ignore"):
        return float(np.min(np.where(bound > 0, value / np.where(bound > 0, bound, 1.0), np.inf)))


def learn(n, w, fwd, nxt, rew, gam, alp, mutant=0):
    """The update behind a step to nxt (Ref [d]) with reward rew (Ref scalar): dict(weights Ref [n, NETD], td Ref,
    better, actor_updates, edge: the smallest distance, in bounds, of td and of the critic's z at s' from 0)."""
    m, d = n - 1, 2 * n + 2
    gam, alp = LD(gam), LD(alp)

    def value_at(vec):
        z = hidden(vec, nxt)
        return output(vec, z)[0], z

    def td_of(v_new):
        gv = gam * v_new.value
        s1 = rew.value + gv
        td = s1 - fwd["out"][m].value
        return Ref(td, rew.bound + abs(float(gam)) * v_new.bound + fwd["out"][m].bound
                   + U * (abs(float(gv)) + abs(float(s1)) + abs(float(td))))

    def stepped(td):
        st = alp * td.value
        return Ref(st, abs(float(alp)) * td.bound + U * abs(float(st)))
    v_new, z_new = value_at(w[m])
    td = td_of(v_new)
    xg = nxt.value if mutant == 5 else fwd["x"].value
    if mutant == 2:
        after = _updated(w[m], stepped(td), xg, fwd["h"][m], fwd["on"][m], 0).value.astype(np.float64)
        td = td_of(value_at(after)[0])
    better = bool(td.value > 0) or mutant == 3
    out = [None] * n
    out[m] = _updated(w[m], stepped(td), xg, fwd["h"][m], fwd["on"][m], mutant)
    for i in range(m):
        if better:
            a, o = fwd["action"], fwd["out"][i]
            diff = a.value[i] if mutant == 6 else a.value[i] - o.value
            sa = alp * diff
            e = abs(float(alp)) * (a.bound[i] + o.bound + U * abs(float(diff)))
            out[i] = _updated(w[i], Ref(sa, e + U * abs(float(sa))), xg, fwd["h"][i], fwd["on"][i], mutant)
        else:
            out[i] = Ref(_ld(w[i]), np.zeros(net_doubles(n)))
    return dict(weights=Ref(np.stack([o.value for o in out]), np.stack([o.bound for o in out])), td=td, better=better,
                actor_updates=int(better),
                edge=min(_edge(td.value, td.bound), _edge(z_new.value, z_new.bound)))


def step(n, w, state, noise, gam, alp, real=(1.0, 1.0, 10.0), h=1e-3, direction=(1.0, 0.0), train=True, mutant=0,
         gate=None):
    """One step of one agent.  w [n, NETD], state [d], noise [n - 1]: exact doubles.  gate: None, or dict(sims [E, 3],
    kind, index, sim_thresh, real_thresh).  -> dict: reward Ref, state Ref [d], weights Ref [n, NETD], actor_updates,
    td Ref (None when nothing learns), edge (the step's decisions: every z, td, both thresholds -- the smallest
    distance from an edge in units of the bound), and with a gate: costs Ref [E], member_in bool [E], admitted, worst
    Ref, and on an admitted step c_real Ref and violation."""
    w = np.asarray(w, dtype=np.float64)
    fwd = forward(n, w, state, noise)
    res = dict(forward=fwd, edge=min(_edge(z.value, z.bound) for z in fwd["z"]))
    admitted = True
    if gate is not None:
        look, _ = physics(gate["sims"], h, direction, state, fwd["action"])
        c = cost(look, gate["kind"], gate["index"])
        with np.errstate(invalid="ignore"):
            member_in = np.asarray(c.value <= LD(gate["sim_thresh"]))
        admitted = bool(member_in.all())
        worst = int(np.argmax(c.value))
        res.update(costs=c, member_in=member_in, admitted=admitted, worst=Ref(c.value[worst], float(c.bound.max())))
        if not np.isnan(gate["sim_thresh"]):
            res["edge"] = min(res["edge"], _edge(c.value - LD(gate["sim_thresh"]), c.bound))
    if not admitted:
        res.update(reward=None, state=Ref(_ld(state), np.zeros(2 * n + 2)),
                   weights=Ref(_ld(w), np.zeros(w.shape)), actor_updates=0, td=None)
        return res
    nxt, rew = physics([real], h, direction, state, fwd["action"])
    nxt, rew = Ref(nxt.value[0], nxt.bound[0]), Ref(rew.value[0], float(rew.bound[0]))
    res.update(reward=rew, state=nxt)
    if gate is not None:
        cr = cost(nxt, gate["kind"], gate["index"])
        res.update(c_real=cr, violation=bool(cr.value > LD(gate["real_thresh"])))
        if not np.isnan(gate["real_thresh"]):
            res["edge"] = min(res["edge"], _edge(cr.value - LD(gate["real_thresh"]), cr.bound))
    if train:
        lr = learn(n, w, fwd, nxt, rew, gam, alp, mutant)
        res.update(weights=lr["weights"], actor_updates=lr["actor_updates"], td=lr["td"],
                   edge=min(res["edge"], lr["edge"]))
    else:
        res.update(weights=Ref(_ld(w), np.zeros(w.shape)), actor_updates=0, td=None)
    return res
