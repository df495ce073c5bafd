"""The checked wrapper of sw_rlglue_ars_run_f64 (include/swimmer_hip.h): device tensors in, ONE foreign call.  It
lives here, next to the classes that use it, and goes through the argument checks of swimmer_amd.kernels: dtype, exact
shape, contiguity and the device of the call's first required tensor, a SwimmerHipError that names the parameter.
Also reachable as swimmer_amd.kernels.rlglue_ars_run."""
import ctypes

import torch

from ..kernels import _gpu, _Min, _out, _tensor
from .._lib import SwParams, check, load, ptr, require_gpu, stream_ptr

_I32 = torch.int32


def rlglue_ars_run(p: SwParams, max_u: float, iter_begin: int, n_iter: int, N: int, b: int, H: int, alpha, nu, deltas,
                   policy, carry, status, eval_returns=None, train_returns=None):
    """n_iter iterations of the RL-Glue ARS experiment on the twin model for A independent agents in ONE launch
    (sw_rlglue_ars_run_f64), one agent per lane.  Every tensor is agent-minor: alpha, nu [A], deltas
    [n_iter, N, m, d, A] (this call's draws), policy [m, d, A], carry [m + 1, A] (stale action, running return; read only
    when iter_begin > 0) and status int32 [A] are updated in place.  Returns (eval_returns [n_iter, A], train_returns
    [n_iter, 2N, A])."""
    require_gpu()
    on = _gpu(alpha, "alpha", 1)
    A = _tensor(alpha, "alpha", (_Min(1),), on).shape[0]
    _tensor(nu, "nu", (A,), on)
    _tensor(deltas, "deltas", (n_iter, N, p.m, p.d, A), on)
    _tensor(policy, "policy", (p.m, p.d, A), on)
    _tensor(carry, "carry", (p.m + 1, A), on)
    _tensor(status, "status", (A,), on, _I32)
    eval_returns = _out(eval_returns, "eval_returns", (n_iter, A), on)
    train_returns = _out(train_returns, "train_returns", (n_iter, 2 * N, A), on)
    check(load().sw_rlglue_ars_run_f64(ctypes.byref(p), float(max_u), A, int(iter_begin), int(n_iter), int(N), int(b),
                                       int(H), ptr(alpha), ptr(nu), ptr(deltas), ptr(policy), ptr(carry),
                                       ptr(eval_returns), ptr(train_returns), ptr(status), stream_ptr()),
          "sw_rlglue_ars_run_f64")
    return eval_returns, train_returns
