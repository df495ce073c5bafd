"""The checked wrapper of sw_safe_ars_rollouts_ensemble_f64 (include/swimmer_hip.h): device tensors in, ONE foreign
call.  It lives here, next to the class that uses it (like ars/ensemble_kernels.py and cacla/safe_kernels.py), goes
through the argument checks of swimmer_amd.kernels -- dtype, exact shape, contiguity and the device of the call's first
required tensor, a SwimmerHipError that names the parameter -- and is reachable as
swimmer_amd.kernels.safe_ars_rollouts_ensemble as well."""
import ctypes

import torch

from ..kernels import _Min, _multi_shapes, _opt, _out, _tensor
from .._lib import SwParams, check, load, ptr, require_gpu, stream_ptr

_I32 = torch.int32


def safe_ars_rollouts_ensemble(p_real: SwParams, H: int, policy, deltas, nu: float, gated, sims, sim_thresh,
                               real_thresh, cost_kind: int, cost_index: int, returns=None, cost_trace=None,
                               cost_max=None, first_refused=None, violations=None, status=None, worst_max=None,
                               refusing_members=None):
    """kernels.safe_ars_rollouts_multi with the per-step gate of a gated agent in an ENSEMBLE of simulators
    (sw_safe_ars_rollouts_ensemble_f64): sims [A, E, 3] = every agent's E members (l_i, m_i, k), 1 <= E <= 64, and a
    step is taken only where every member's cost is <= sim_thresh.  Everything else as safe_ars_rollouts_multi, in the
    arithmetic of its lane form.  Two more optional outputs, filled when given: worst_max [A, 2N], the largest member
    cost over the admitted steps (0 where none was admitted, NaN for an ungated agent), and refusing_members int64
    [A, 2N], bit e set iff member e refused the first refused step (0: none refused).  A gated agent with a member
    that breaks the parameter rule: SW_STATUS_PARAM, NaN returns, first_refused 0, the bad members' bits."""
    require_gpu()
    A, N, on = _multi_shapes(p_real, policy, deltas, None, None)
    _tensor(gated, "gated", (A,), on, _I32)
    E = _tensor(sims, "sims", (A, _Min(1), 3), on).shape[1]
    _tensor(sim_thresh, "sim_thresh", (A,), on)
    _tensor(real_thresh, "real_thresh", (A,), on)
    _opt(cost_trace, "cost_trace", (H, A, 2 * N), on)
    for name, t in (("cost_max", cost_max), ("worst_max", worst_max)):
        _opt(t, name, (A, 2 * N), on)
    for name, t in (("first_refused", first_refused), ("violations", violations), ("status", status)):
        _opt(t, name, (A, 2 * N), on, _I32)
    _opt(refusing_members, "refusing_members", (A, 2 * N), on, torch.int64)
    returns = _out(returns, "returns", (A, 2 * N), on)
    check(load().sw_safe_ars_rollouts_ensemble_f64(ctypes.byref(p_real), A, E, N, H, ptr(policy), ptr(deltas),
                                                   float(nu), ptr(gated), ptr(sims), ptr(sim_thresh), ptr(real_thresh),
                                                   int(cost_kind), int(cost_index), ptr(returns), ptr(cost_trace),
                                                   ptr(cost_max), ptr(first_refused), ptr(violations), ptr(status),
                                                   ptr(worst_max), ptr(refusing_members), stream_ptr()),
          "sw_safe_ars_rollouts_ensemble_f64")
    return returns
