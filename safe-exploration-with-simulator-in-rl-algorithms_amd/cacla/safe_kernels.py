"""The checked wrappers of sw_cacla_safe_run_f64 and sw_cacla_safe_ensemble_run_f64 (include/swimmer_hip.h): device
tensors in, ONE foreign call each.  They live here, next to the classes that use them, and go through the argument
checks of swimmer_amd.kernels: dtype, exact shape, contiguity and the device of the call's first required tensor, a
SwimmerHipError that names the parameter."""
import ctypes

import torch

from ..kernels import _gpu, _Min, _opt, _out, _tensor, cacla_net_doubles
from .._lib import STATUS_PARAM, SwParams, check, load, ptr, require_gpu, stream_ptr  # noqa: F401

_I32 = torch.int32


def _gated_args(p, n_iter, gamma, alpha, noise, gated, sims, sims_name, sims_shape, sim_thresh, real_thresh, weights,
                state, last_reward, counters, first_refused, admitted_rec):
    """The tensor checks both wrappers share, in the order the library takes the arguments; the simulators' array is
    [A, *sims_shape].  -> (the call's device, A)."""
    on = _gpu(gamma, "gamma", 1)
    A = _tensor(gamma, "gamma", (_Min(1),), on).shape[0]
    _tensor(alpha, "alpha", (A,), on)
    _tensor(noise, "noise", (A, n_iter, p.m), on)
    _tensor(gated, "gated", (A,), on, _I32)
    _tensor(sims, sims_name, (A,) + sims_shape, on)
    _tensor(sim_thresh, "sim_thresh", (A,), on)
    _tensor(real_thresh, "real_thresh", (A,), on)
    _tensor(weights, "weights", (A, p.n, cacla_net_doubles(p.n)), on)
    _tensor(state, "state", (A, p.d), on)
    _tensor(last_reward, "last_reward", (A,), on)
    _tensor(counters, "counters", (A, 3), on, _I32)
    _tensor(first_refused, "first_refused", (A,), on, _I32)
    _opt(admitted_rec, "admitted_rec", (A, n_iter), on, _I32)
    return on, A


def cacla_safe_run(p: SwParams, n_iter: int, t_begin: int, gamma, alpha, noise, gated, sim, sim_thresh, real_thresh,
                   cost_kind: int, cost_index: int, weights, state, last_reward, counters, first_refused,
                   rewards=None, admitted_rec=None, status=None):
    """n_iter steps of CACLA behind the simulator gate for A independent agents in ONE launch
    (sw_cacla_safe_run_f64), one wave per agent: gamma, alpha [A], noise [A, n_iter, m], gated int32 [A], sim [A, 3]
    (l_i, m_i, k), sim_thresh / real_thresh [A]; weights [A, n, cacla_net_doubles(n)], state [A, d], last_reward [A]
    (NaN before a run), counters int32 [A, 3] (admitted, violations, actor updates; zero before a run) and
    first_refused int32 [A] (-1 before a run) updated in place; admitted_rec int32 [A, n_iter] and status int32 [A]
    written / accumulated when given.  t_begin: the steps of the run already taken (first_refused counts from the
    run's start).  Returns `rewards` [A, n_iter]: the last admitted step's reward, NaN before the first admission."""
    require_gpu()
    on, A = _gated_args(p, n_iter, gamma, alpha, noise, gated, sim, "sim", (3,), sim_thresh, real_thresh, weights,
                        state, last_reward, counters, first_refused, admitted_rec)
    _opt(status, "status", (A,), on, _I32)
    rewards = _out(rewards, "rewards", (A, n_iter), on)
    check(load().sw_cacla_safe_run_f64(ctypes.byref(p), A, int(n_iter), int(t_begin), ptr(gamma), ptr(alpha),
                                       ptr(noise), ptr(gated), ptr(sim), ptr(sim_thresh), ptr(real_thresh),
                                       int(cost_kind), int(cost_index), ptr(weights), ptr(state), ptr(last_reward),
                                       ptr(rewards), ptr(admitted_rec), ptr(counters), ptr(first_refused), ptr(status),
                                       stream_ptr()), "sw_cacla_safe_run_f64")
    return rewards


def cacla_safe_ensemble_run(p: SwParams, n_iter: int, t_begin: int, gamma, alpha, noise, gated, sims, sim_thresh,
                            real_thresh, cost_kind: int, cost_index: int, weights, state, last_reward, counters,
                            first_refused, rewards=None, admitted_rec=None, worst_rec=None, member_refusals=None,
                            status=None):
    """cacla_safe_run with every step gated on an ENSEMBLE of simulators (sw_cacla_safe_ensemble_run_f64): sims
    [A, E, 3] rows (l_i, m_i, k), the same E for every agent, at most 64 (the library's SW_ERR_SIZE beyond), and a
    step is taken only where every member admits it.  Everything else as cacla_safe_run; besides, when given,
    worst_rec [A, n_iter] is written (the largest member cost of each step, NaN or a bad member as +inf; NaN for an
    ungated agent) and member_refusals int32 [A, E] (zero before a run) accumulates the steps at which each member's
    own cost was not <= sim_thresh.  Returns `rewards` [A, n_iter]."""
    require_gpu()
    on, A = _gated_args(p, n_iter, gamma, alpha, noise, gated, sims, "sims", (_Min(1), 3), sim_thresh, real_thresh,
                        weights, state, last_reward, counters, first_refused, admitted_rec)
    E = sims.shape[1]
    _opt(worst_rec, "worst_rec", (A, n_iter), on)
    _opt(member_refusals, "member_refusals", (A, E), on, _I32)
    _opt(status, "status", (A,), on, _I32)
    rewards = _out(rewards, "rewards", (A, n_iter), on)
    check(load().sw_cacla_safe_ensemble_run_f64(ctypes.byref(p), A, E, int(n_iter), int(t_begin), ptr(gamma),
                                                ptr(alpha), ptr(noise), ptr(gated), ptr(sims), ptr(sim_thresh),
                                                ptr(real_thresh), int(cost_kind), int(cost_index), ptr(weights),
                                                ptr(state), ptr(last_reward), ptr(rewards), ptr(admitted_rec),
                                                ptr(worst_rec), ptr(member_refusals), ptr(counters),
                                                ptr(first_refused), ptr(status), stream_ptr()),
          "sw_cacla_safe_ensemble_run_f64")
    return rewards
