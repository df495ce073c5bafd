"""The checked wrapper of sw_ars_gate_ensemble_f64 (include/swimmer_hip.h): device tensors in, ONE foreign call.  It
lives here, next to the classes that use it, and goes through the argument checks of swimmer_amd.kernels: dtype, exact
shape, contiguity and the device of the call's first required tensor, a SwimmerHipError that names the parameter."""
import ctypes

import torch

from ..kernels import _gpu, _Min, _opt, _out, _pair, _tensor
from .._lib import SwParams, check, load, ptr, require_gpu, stream_ptr

_I32 = torch.int32


def ars_gate_ensemble(p_base: SwParams, H: int, policy, deltas, nu: float, sim, sim_thresh, mean=None, inv_std=None,
                      admit=None, worst=None, status=None, member_returns=None, member_status=None,
                      member_admit=None):
    """The simulator gate of S agents in E simulators each, and the fold over them, in ONE call
    (sw_ars_gate_ensemble_f64: the member launch, then the fold): policy [S, m, d], deltas [S, N, m, d], mean /
    inv_std [S, d] (both or neither) and sim_thresh [S] per agent, shared by the agent's members; sim [S, E, 3] = member
    e's (l_i, m_i, k); n, h, the direction and the flags of every simulator come from p_base.  Returns (admit, worst):
    admit int32 [S, N], 1 where EVERY member admits the direction; worst [S, 2N], the smallest of the members' returns
    (a NaN never counts; +inf where all are NaN).  status (int32 [S, 2N], optional) receives the OR of the members'
    status; member_returns / member_status ([S, E, 2N]) and member_admit (int32 [S, E, N]) are what ars_gate gives for
    agent a in simulator e, allocated here when not given: the fold reads them.  A member that breaks the parameter
    rule: SW_STATUS_PARAM, and its agent admits nothing."""
    require_gpu()
    on = _gpu(policy, "policy", 3)
    S = _tensor(policy, "policy", (_Min(1), p_base.m, p_base.d), on).shape[0]
    N = _tensor(deltas, "deltas", (S, _Min(1), p_base.m, p_base.d), on).shape[1]
    _pair(mean, inv_std, (S, p_base.d), on)
    E = _tensor(sim, "sim", (S, _Min(1), 3), on).shape[1]
    _tensor(sim_thresh, "sim_thresh", (S,), on)
    admit = _out(admit, "admit", (S, N), on, _I32)
    worst = _out(worst, "worst", (S, 2 * N), on)
    _opt(status, "status", (S, 2 * N), on, _I32)
    member_returns = _out(member_returns, "member_returns", (S, E, 2 * N), on)
    member_status = _out(member_status, "member_status", (S, E, 2 * N), on, _I32)
    member_admit = _out(member_admit, "member_admit", (S, E, N), on, _I32)
    check(load().sw_ars_gate_ensemble_f64(ctypes.byref(p_base), S, E, N, H, ptr(policy), ptr(deltas), float(nu),
                                          ptr(mean), ptr(inv_std), ptr(sim), ptr(sim_thresh), ptr(admit), ptr(worst),
                                          ptr(status), ptr(member_returns), ptr(member_status), ptr(member_admit),
                                          stream_ptr()), "sw_ars_gate_ensemble_f64")
    return admit, worst
