"""Ensembles of simulators for the safe-ARS gate, and the NumPy restatement of the gate's fold.  Host side only.

The reference leaves its simulator threshold open: `threshold + alpha(H) * epsilon` with Lipschitz constants K, A, B
that nobody knows (ars/ars_agent.py:59-70, `# TODO compute sim_threshold`; its main script sweeps A over four guesses).
The ensemble gate (sw_ars_gate_ensemble_f64, ars/ensemble_kernels.py) needs none of them: the gate runs in E
simulators that stand for the uncertainty about the real parameters -- the estimates of an EstimatorBatch over subsets
and seeds (ensemble_from_estimates), or samples on the epsilon-sphere around one estimate (sphere_ensemble) -- and a
direction is admitted only where EVERY one admits it.  The worst simulated return takes the place of alpha * epsilon.

The rule, used by the kernels, the agents and fold_reference alike.  Member e of an agent runs the 2N rollouts
P +- nu delta_j in simulator e, as ars_gate does:

    member_admit[e][j] = !(r+ <= thr) && !(r- <= thr)    equality refuses; a NaN return or a NaN threshold admits
    admit[j]           = AND over e of member_admit[e][j]
    worst[r]           = min over e of member e's return r, taken as w = (x < w) ? x : w from +inf in ascending e:
                         a NaN never replaces w, and where every member's return is NaN worst is +inf
    status[r]          = bitwise OR over e of the members' status (the SW_STATUS_* codes are bit flags)

A member whose (l_i, m_i, k) breaks the parameter rule has SW_STATUS_PARAM, NaN returns and admits nothing, so its
agent admits nothing.  Where status[2j] | status[2j+1] == 0, admit[j] == !(worst[2j] <= thr) && !(worst[2j+1] <= thr):
a refusing member holds a return <= thr, which the minimum then is too, and an admitting ensemble holds none.  (The
one input outside it is hand-made: every member's return NaN under a status of 0 against thr = +inf -- the members
admit, worst = +inf does not.  A rollout of the kernels whose return is NaN has a non-zero status.)
"""
import copy
import math

import numpy as np

from .._lib import STATUS_PARAM
from .parameters import EnvParam

UNKNOWNS = ('m_i', 'l_i', 'k')    # the reference's order (ars/ars_agent.py:46, ars/estimator.py)


def params_ok(p):
    """The parameter rule of the library for the three unknowns of an EnvParam."""
    return bool(p.l_i > 0 and p.m_i > 0 and math.isfinite(p.l_i) and math.isfinite(p.m_i) and math.isfinite(p.k))


def sphere_ensemble(center, epsilon, n_sim, rng=None):
    """n_sim simulators on the epsilon-sphere around `center` (an EnvParam): member 0 is a copy of the centre, member
    i >= 1 the centre with (m_i, l_i, k) += epsilon * g / ||g||_2, g = rng.standard_normal(3) drawn in member order
    from `rng` (a RandomState; default: NumPy's global generator) -- a normalised Gaussian is uniform on the sphere.
    `center` is not touched."""
    n_sim = int(n_sim)
    if n_sim < 1:
        raise ValueError("sphere_ensemble needs n_sim >= 1")
    normal = np.random.standard_normal if rng is None else rng.standard_normal
    out = [copy.copy(center)]
    for _ in range(1, n_sim):
        g = normal(3)
        step = epsilon * (g / np.linalg.norm(g, ord=2))
        sim = copy.copy(center)
        for name, s in zip(UNKNOWNS, step):
            setattr(sim, name, getattr(center, name) + float(s))
        out.append(sim)
    return out


def ensemble_from_estimates(estimates, like=None):
    """The estimates of an EstimatorBatch -- EnvParams (EstimatorBatch.estimate) or rows [m_i, l_i, k] next to `like`,
    an EnvParam that gives everything else -- as an ensemble: a list of EnvParam without the rows that break the
    parameter rule (a search that ran away must not silence the whole gate).  ValueError when none remain."""
    out = []
    for e in estimates:
        if not isinstance(e, EnvParam):
            if like is None:
                raise ValueError("ensemble_from_estimates: rows [m_i, l_i, k] need `like`, an EnvParam for the rest")
            row = [float(v) for v in e]
            if len(row) != len(UNKNOWNS):
                raise ValueError(f"ensemble_from_estimates: a row holds {UNKNOWNS}, got {len(row)} values")
            e = copy.copy(like)
            for name, v in zip(UNKNOWNS, row):
                setattr(e, name, v)
        if params_ok(e):
            out.append(copy.copy(e))
    if not out:
        raise ValueError("ensemble_from_estimates: no estimate satisfies the parameter rule (l_i, m_i > 0, finite)")
    return out


def check_ensemble(ensemble, real_env_param, what="sim_ensemble"):
    """An ensemble an agent can gate with: a non-empty list of EnvParam with the real world's n, h and H -> the list.
    (A member that breaks the parameter rule is the kernels' business: SW_STATUS_PARAM.)"""
    ensemble = list(ensemble)
    if not ensemble:
        raise ValueError(f"{what}: an ensemble needs at least one simulator")
    for e, sp in enumerate(ensemble):
        if sp.n != real_env_param.n or sp.h != real_env_param.h or sp.H != real_env_param.H:
            raise ValueError(f"{what}[{e}]: n = {sp.n}, h = {sp.h}, H = {sp.H}; the members share the real world's "
                             f"n = {real_env_param.n}, h = {real_env_param.h} and H = {real_env_param.H}")
    return ensemble


def sim_rows(ensemble):
    """[E, 3] (l_i, m_i, k): the rows sw_ars_gate_ensemble_f64 reads."""
    return np.array([[sp.l_i, sp.m_i, sp.k] for sp in ensemble], dtype=np.float64)


def fold_reference(member_returns, member_status, thr):
    """The rule above in NumPy, for tests (the product never calls it): member_returns [..., E, 2N], member_status
    [..., E, 2N] (int), thr a scalar or [...] -> (member_admit [..., E, N], admit [..., N], worst [..., 2N],
    status [..., 2N]); the flags and the status are int32."""
    r = np.asarray(member_returns, dtype=np.float64)
    st = np.asarray(member_status).astype(np.int32)
    lead, E, n_roll = r.shape[:-2], r.shape[-2], r.shape[-1]
    t = np.broadcast_to(np.asarray(thr, dtype=np.float64), lead)[..., None, None]
    with np.errstate(invalid="ignore"):
        passes = ~(r <= t)                                            # False for a NaN on either side: admits
    member_admit = passes[..., 0::2] & passes[..., 1::2]
    member_admit &= ~((st[..., 0::2] | st[..., 1::2]) & STATUS_PARAM).astype(bool)   # a bad member admits nothing
    worst = np.full(lead + (n_roll,), np.inf)
    status = np.zeros(lead + (n_roll,), dtype=np.int32)
    for e in range(E):                                                # ascending, as the kernel walks them
        x = r[..., e, :]
        with np.errstate(invalid="ignore"):
            worst = np.where(x < worst, x, worst)
        status |= st[..., e, :]
    return member_admit.astype(np.int32), member_admit.all(axis=-2).astype(np.int32), worst, status
