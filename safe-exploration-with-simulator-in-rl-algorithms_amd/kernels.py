"""Functional wrappers: torch device tensors in, one C-ABI call (include/swimmer_hip.h) each.

Shapes follow the ABI: states are SoA [d, n_env], actions [m, n_env], policies AoS
[n_roll, m, d], trajectories [H, d, n_roll].  Everything is float64 and stays on the GPU;
all calls are asynchronous on torch's current stream.
"""
import ctypes

import torch

from . import _lib
from ._lib import SwParams, check, load, ptr, require_gpu, stream_ptr


def _f64(shape, device):
    return torch.empty(shape, dtype=torch.float64, device=device)


def _want(t, name, shape):
    if t.dtype != torch.float64 or tuple(t.shape) != tuple(shape):
        raise _lib.SwimmerHipError(f"{name}: expected float64 tensor of shape {tuple(shape)}, "
                                   f"got {t.dtype} {tuple(t.shape)}")
    return t


def reset(p: SwParams, n_env: int, device="cuda:0", out=None):
    """SwimmerEnv.reset for n_env swimmers -> state [d, n_env]."""
    require_gpu()
    state = _f64((p.d, n_env), device) if out is None else _want(out, "out", (p.d, n_env))
    check(load().sw_reset_f64(ctypes.byref(p), n_env, ptr(state), stream_ptr()), "sw_reset_f64")
    return state


def step(p: SwParams, state, action, out=None, reward=None, status=None):
    """One physics step.  Returns (next_state [d, n_env], reward [n_env])."""
    require_gpu()
    n_env = state.shape[1]
    _want(state, "state", (p.d, n_env))
    _want(action, "action", (p.m, n_env))
    out = _f64((p.d, n_env), state.device) if out is None else _want(out, "out", (p.d, n_env))
    reward = _f64((n_env,), state.device) if reward is None else _want(reward, "reward", (n_env,))
    check(load().sw_step_f64(ctypes.byref(p), n_env, ptr(state), ptr(action), ptr(out),
                             ptr(reward), ptr(status), stream_ptr()), "sw_step_f64")
    return out, reward


def step_residual_blocks(n_transitions: int) -> int:
    return int(load().sw_step_residual_blocks(int(n_transitions)))


def step_residual(p: SwParams, state, action, next_ref, partial=None):
    """Estimator.I's inner sum (ars/estimator.py:36-62) in one pass: per-workgroup sums of
    || step(state, action) - next_ref ||_2 over the transitions (SoA [d, T], [m, T], [d, T]); their sum is I(x).
    The simulated next states are never written (sw_step_residual_f64)."""
    require_gpu()
    T = state.shape[1]
    _want(state, "state", (p.d, T))
    _want(action, "action", (p.m, T))
    _want(next_ref, "next_ref", (p.d, T))
    nb = int(load().sw_step_residual_blocks(T))
    partial = _f64((nb,), state.device) if partial is None else _want(partial, "partial", (nb,))
    check(load().sw_step_residual_f64(ctypes.byref(p), T, ptr(state), ptr(action), ptr(next_ref), ptr(partial),
                                      stream_ptr()), "sw_step_residual_f64")
    return partial


def step_residual_population(p_base: SwParams, cand, state, action, next_ref, partial=None, value=None, status=None):
    """step_residual for a whole population of parameter sets in one launch (sw_step_residual_pop_f64): cand
    [n_cand, 3] float64 holds each candidate's (l_i, m_i, k) on the device; n, h and the direction come from p_base.
    Returns (value [n_cand], partial [n_cand, step_residual_blocks(T)], status [n_cand] int32): partial row j has the
    bits step_residual gives for candidate j, value[j] is its fixed-order sum, status[j] is SW_STATUS_PARAM (8) for
    a candidate with non-positive / non-finite l_i, m_i or non-finite k (NaN partials and value), else 0."""
    require_gpu()
    T = state.shape[1]
    _want(state, "state", (p_base.d, T))
    _want(action, "action", (p_base.m, T))
    _want(next_ref, "next_ref", (p_base.d, T))
    if cand.dim() != 2 or cand.shape[0] < 1:
        raise _lib.SwimmerHipError(f"cand: expected float64 tensor of shape (n_cand, 3), got {tuple(cand.shape)}")
    n_cand = cand.shape[0]
    _want(cand, "cand", (n_cand, 3))
    if not cand.is_contiguous():
        raise _lib.SwimmerHipError("cand: expected a contiguous tensor")
    nb = int(load().sw_step_residual_blocks(T))
    partial = _f64((n_cand, nb), state.device) if partial is None else _want(partial, "partial", (n_cand, nb))
    if value is None:   # zeros: with T = 0 the library writes nothing and I is 0
        value = torch.zeros((n_cand,), dtype=torch.float64, device=state.device)
    else:
        _want(value, "value", (n_cand,))
    if status is None:
        status = torch.zeros((n_cand,), dtype=torch.int32, device=state.device)
    elif status.dtype != torch.int32 or tuple(status.shape) != (n_cand,):
        raise _lib.SwimmerHipError(f"status: expected int32 tensor of shape ({n_cand},)")
    check(load().sw_step_residual_pop_f64(ctypes.byref(p_base), n_cand, ptr(cand), T, ptr(state), ptr(action),
                                          ptr(next_ref), ptr(partial), ptr(value), ptr(status), stream_ptr()),
          "sw_step_residual_pop_f64")
    return value, partial, status


def _want_typed(t, name, dtype, shape):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise _lib.SwimmerHipError(f"{name}: expected a contiguous {dtype} tensor of shape {tuple(shape)}, "
                                   f"got {t.dtype} {tuple(t.shape)}")
    return t


def _sets_shapes(p_base, set_begin, max_set_len, state, action, next_ref):
    T = state.shape[1]
    _want(state, "state", (p_base.d, T))
    _want(action, "action", (p_base.m, T))
    _want(next_ref, "next_ref", (p_base.d, T))
    if set_begin.dim() != 1 or set_begin.shape[0] < 2:
        raise _lib.SwimmerHipError(f"set_begin: expected int64 tensor of shape (n_set + 1,), got {tuple(set_begin.shape)}")
    n_set = set_begin.shape[0] - 1
    _want_typed(set_begin, "set_begin", torch.int64, (n_set + 1,))
    return T, n_set, int(load().sw_step_residual_blocks(int(max_set_len)))


def step_residual_sets(p_base: SwParams, set_begin, max_set_len: int, cand, cand_set, state, action, next_ref,
                       partial=None, value=None, status=None):
    """step_residual_population for candidates that score on different transition sets, in one launch
    (sw_step_residual_sets_f64): set s is columns [set_begin[s], set_begin[s + 1]) of the concatenated transitions
    (set_begin int64 [n_set + 1] on the device, max_set_len the longest set), candidate j = cand[j] (l_i, m_i, k)
    scores on set cand_set[j] (int32 [n_cand], ascending).  Returns (value [n_cand], partial [n_cand,
    step_residual_blocks(max_set_len)], status [n_cand]): the first step_residual_blocks(len of j's set) entries of
    partial[j] have the bits step_residual gives for candidate j on its set's slice (the rest is not written),
    value[j] is their fixed-order sum."""
    require_gpu()
    T, n_set, nb = _sets_shapes(p_base, set_begin, max_set_len, state, action, next_ref)
    if cand.dim() != 2 or cand.shape[0] < 1:
        raise _lib.SwimmerHipError(f"cand: expected float64 tensor of shape (n_cand, 3), got {tuple(cand.shape)}")
    n_cand = cand.shape[0]
    _want_typed(cand, "cand", torch.float64, (n_cand, 3))
    _want_typed(cand_set, "cand_set", torch.int32, (n_cand,))
    partial = _f64((n_cand, nb), state.device) if partial is None else _want(partial, "partial", (n_cand, nb))
    value = _f64((n_cand,), state.device) if value is None else _want(value, "value", (n_cand,))
    if status is None:
        status = torch.zeros((n_cand,), dtype=torch.int32, device=state.device)
    else:
        _want_typed(status, "status", torch.int32, (n_cand,))
    check(load().sw_step_residual_sets_f64(ctypes.byref(p_base), n_set, ptr(set_begin), int(max_set_len), n_cand,
                                           ptr(cand), ptr(cand_set), T, ptr(state), ptr(action), ptr(next_ref),
                                           ptr(partial), ptr(value), ptr(status), stream_ptr()),
          "sw_step_residual_sets_f64")
    return value, partial, status


def step_residual_normal_sets(p_base: SwParams, set_begin, max_set_len: int, points, state, action, next_ref,
                              inv_2e=None, active=None, partial=None, out=None, status=None):
    """The least-squares refinement's sums per transition set, fused (sw_step_residual_normal_sets_f64): points
    [n_set, n_point, 3] = (l_i, m_i, k).  n_point = 1: out [n_set, 1] = r.r with r = step - next_ref over the set;
    n_point = 7 (centre, +e0, -e0, +e1, -e1, +e2, -e2, with inv_2e [n_set, 3]): out [n_set, 13] = r.r | J^T J | J^T r,
    J by central differences.  active (int32 [n_set]): sets with 0 are neither read nor written.  Returns (out,
    status [n_set])."""
    require_gpu()
    T, n_set, nb = _sets_shapes(p_base, set_begin, max_set_len, state, action, next_ref)
    if points.dim() != 3:
        raise _lib.SwimmerHipError(f"points: expected float64 tensor of shape (n_set, n_point, 3), got "
                                   f"{tuple(points.shape)}")
    n_point = points.shape[1]
    _want_typed(points, "points", torch.float64, (n_set, n_point, 3))
    K = 13 if n_point == 7 else 1
    if inv_2e is not None:
        _want_typed(inv_2e, "inv_2e", torch.float64, (n_set, 3))
    if active is not None:
        _want_typed(active, "active", torch.int32, (n_set,))
    partial = _f64((n_set, K, nb), state.device) if partial is None else _want(partial, "partial", (n_set, K, nb))
    out = _f64((n_set, K), state.device) if out is None else _want(out, "out", (n_set, K))
    if status is None:
        status = torch.zeros((n_set,), dtype=torch.int32, device=state.device)
    else:
        _want_typed(status, "status", torch.int32, (n_set,))
    check(load().sw_step_residual_normal_sets_f64(ctypes.byref(p_base), n_set, ptr(set_begin), int(max_set_len),
                                                  n_point, ptr(points), ptr(inv_2e), ptr(active), T, ptr(state),
                                                  ptr(action), ptr(next_ref), ptr(partial), ptr(out), ptr(status),
                                                  stream_ptr()), "sw_step_residual_normal_sets_f64")
    return out, status


class StepPlan(object):
    """A pre-bound sw_step_f64 launch: all argument conversion is done once, `launch()` is a
    single foreign call (the per-launch Python overhead of `step()` is larger than the 8192-env
    kernel itself).  Launches on the stream that was current when the plan was made."""

    def __init__(self, p: SwParams, state, action, out, reward=None, status=None):
        require_gpu()
        n_env = state.shape[1]
        _want(state, "state", (p.d, n_env))
        _want(action, "action", (p.m, n_env))
        _want(out, "out", (p.d, n_env))
        if reward is not None:
            _want(reward, "reward", (n_env,))
        self._keep = (p, state, action, out, reward, status)
        self._fn = load().sw_step_f64
        self._args = (ctypes.byref(p), n_env, ptr(state), ptr(action), ptr(out), ptr(reward),
                      ptr(status), stream_ptr())

    def launch(self):
        rc = self._fn(*self._args)
        if rc:
            check(rc, "sw_step_f64")


class DirectComm(object):
    """sw_comm: the per-iteration all-gather issued straight into RCCL from native code on the
    current stream (no ProcessGroupNCCL in between).  COLLECTIVE constructor: rank 0 draws the
    unique id, `broadcast_id(id_bytes_or_None)` must hand every rank rank 0's 128 bytes, and
    `agree(ok)` (a collective AND over the ranks; identity with one rank) makes a failure on ANY
    rank -- RCCL not resolvable, the id not drawn, the communicator not created -- an exception
    on EVERY rank instead of a hang of the others in the next collective.  The communicator binds
    to the CURRENT device: construct it under `torch.cuda.device(...)`.  EXPERIMENTAL until it has
    met more than one rank."""

    def __init__(self, world, rank, broadcast_id, agree=None):
        require_gpu()
        agree = agree or (lambda ok: ok)
        lib = load()
        why = None
        buf = (ctypes.c_uint8 * 128)()
        if not lib.sw_comm_available():
            why = "RCCL (librccl.so.1) could not be resolved at run time"
        elif rank == 0:
            rc = lib.sw_comm_unique_id(buf)
            if rc:
                why = f"sw_comm_unique_id: {_lib.ERR_NAMES.get(rc, rc)}"
        if not agree(why is None):
            raise _lib.SwimmerHipError("direct RCCL set-up failed on " +
                                       (f"this rank: {why}" if why else "another rank"))
        ident = broadcast_id(bytes(buf) if rank == 0 else None)
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(ident)
        h = ctypes.c_void_p()
        rc = lib.sw_comm_create(ctypes.byref(h), buf, world, rank)
        if not agree(rc == 0):
            if rc == 0:
                lib.sw_comm_destroy(h)
            raise _lib.SwimmerHipError("sw_comm_create failed on " +
                                       (f"this rank: {_lib.ERR_NAMES.get(rc, rc)}" if rc else "another rank"))
        self._h, self._lib, self.world, self.rank = h, lib, world, rank
        self._fn = lib.sw_comm_all_gather_f64

    def all_gather(self, send, gathered):
        """gathered[r * L : (r + 1) * L] <- rank r's send (L = send.numel()), on the current stream."""
        if gathered.numel() != self.world * send.numel():
            raise _lib.SwimmerHipError("all_gather: gathered must hold world x send doubles")
        rc = self._fn(self._h, ptr(send), ptr(gathered), send.numel(), stream_ptr())
        if rc:
            raise _lib.SwimmerHipError("sw_comm_all_gather_f64: " + self._lib.sw_comm_last_error(self._h).decode())
        return gathered

    def close(self):
        if self._h is not None:
            self._lib.sw_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass


class SingleEnv(object):
    """sw_env1: ONE swimmer handed over in host memory -- the batch-1 surface under
    `SwimmerEnv.step` (remy_swimmer_env.py:41-56).  The handle owns a pinned, device-mapped I/O
    block; `io` is a NumPy view of it (offsets SW_ENV1_* of include/swimmer_hip.h).  A step is
    one kernel launch and one host wait: no tensor is created, nothing is copied by a call."""
    STATE, ACTION, NEXT, REWARD, GDD, TDD, DOUBLES = 0, 18, 32, 50, 52, 54, 64

    def __init__(self):
        require_gpu()
        import numpy as np
        lib = load()
        h = ctypes.c_void_p()
        check(lib.sw_env1_create(ctypes.byref(h)), "sw_env1_create")
        self._h, self._lib = h, lib
        self.io = np.ctypeslib.as_array(lib.sw_env1_io(h), shape=(self.DOUBLES,))
        self._status = ctypes.c_int32(0)
        self._step, self._accel = lib.sw_env1_step, lib.sw_env1_accel

    def step(self, p: SwParams):
        """State and action are in `io`; returns the status bits, next state / reward in `io`."""
        rc = self._step(self._h, ctypes.byref(p), ctypes.byref(self._status))
        if rc:
            check(rc, "sw_env1_step")
        return self._status.value

    def accelerations(self, p: SwParams):
        rc = self._accel(self._h, ctypes.byref(p))
        if rc:
            check(rc, "sw_env1_accel")

    def close(self):
        if self._h is not None:
            self.io = None
            self._lib.sw_env1_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass


def accelerations(p: SwParams, state, action):
    """SwimmerEnv.compute_accelerations -> (Gdd [2, n_env], thdd [n, n_env])."""
    require_gpu()
    n_env = state.shape[1]
    _want(state, "state", (p.d, n_env))
    _want(action, "action", (p.m, n_env))
    gdd = _f64((2, n_env), state.device)
    tdd = _f64((p.n, n_env), state.device)
    check(load().sw_accel_f64(ctypes.byref(p), n_env, ptr(state), ptr(action), ptr(gdd),
                              ptr(tdd), stream_ptr()), "sw_accel_f64")
    return gdd, tdd


def moments_blocks(n_roll: int) -> int:
    return int(load().sw_moments_blocks(n_roll))


def rollout(p: SwParams, H: int, policies, mean=None, inv_std=None, state0=None,
            traj=None, final_state=None, moments=None, status=None, returns=None):
    """n_roll H-step rollouts, one linear policy each.  Optional output buffers are filled
    when given (see include/swimmer_hip.h for their shapes).  Returns `returns` [n_roll]."""
    require_gpu()
    n_roll = policies.shape[0]
    _want(policies, "policies", (n_roll, p.m, p.d))
    dev = policies.device
    if (mean is None) != (inv_std is None):
        raise _lib.SwimmerHipError("mean and inv_std must be given together")
    if mean is not None:
        _want(mean, "mean", (p.d,))
        _want(inv_std, "inv_std", (p.d,))
    if state0 is not None:
        _want(state0, "state0", (p.d, n_roll))
    if traj is not None:
        _want(traj, "traj", (H, p.d, n_roll))
    if final_state is not None:
        _want(final_state, "final_state", (p.d, n_roll))
    if moments is not None:
        _want(moments, "moments", (moments_blocks(n_roll), 2 * p.d))
    returns = _f64((n_roll,), dev) if returns is None else _want(returns, "returns", (n_roll,))
    check(load().sw_rollout_f64(ctypes.byref(p), n_roll, H, ptr(policies), ptr(mean),
                                ptr(inv_std), ptr(state0), ptr(returns), ptr(traj),
                                ptr(final_state), ptr(moments), ptr(status), stream_ptr()),
          "sw_rollout_f64")
    return returns


def safe_rollouts(p_real: SwParams, p_sim: SwParams, H: int, policies, cost_kind: int, cost_index: int,
                  sim_thresh: float, real_thresh: float, traj=None, first_refused=None, violations=None,
                  status=None, returns=None):
    """safe_ars/ars.py Safe_ARS.rollout for a whole batch in ONE launch (sw_safe_rollouts_f64): n_roll rollouts of H
    steps from the reset state, every real step gated by the one-step simulator look-ahead (`isSafe`, :111-122).
    policies [n_roll, m, d]; optional outputs: traj [H, d, n_roll], first_refused / violations / status [n_roll] int32."""
    require_gpu()
    n_roll = policies.shape[0]
    _want(policies, "policies", (n_roll, p_real.m, p_real.d))
    dev = policies.device
    if traj is not None:
        _want(traj, "traj", (H, p_real.d, n_roll))
    for name, t in (("first_refused", first_refused), ("violations", violations), ("status", status)):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (n_roll,)):
            raise _lib.SwimmerHipError(f"{name}: expected int32 tensor of shape ({n_roll},)")
    returns = _f64((n_roll,), dev) if returns is None else _want(returns, "returns", (n_roll,))
    check(load().sw_safe_rollouts_f64(ctypes.byref(p_real), ctypes.byref(p_sim), n_roll, H, ptr(policies),
                                      int(cost_kind), int(cost_index), float(sim_thresh), float(real_thresh),
                                      ptr(returns), ptr(traj), ptr(first_refused), ptr(violations), ptr(status),
                                      stream_ptr()), "sw_safe_rollouts_f64")
    return returns


def ars_rollouts(p: SwParams, H: int, policy, deltas, nu: float, dir_begin: int, n_dir: int,
                 mean=None, inv_std=None, returns=None, traj=None, moments=None, status=None):
    """The 2*n_dir exploration rollouts P +- nu*delta_i, i in [dir_begin, dir_begin+n_dir)."""
    require_gpu()
    _want(policy, "policy", (p.m, p.d))
    if deltas.dim() != 3 or deltas.shape[0] < dir_begin + n_dir:
        raise _lib.SwimmerHipError("deltas: need [>= dir_begin + n_dir, m, d]")
    _want(deltas, "deltas", (deltas.shape[0], p.m, p.d))
    dev = policy.device
    n_roll = 2 * n_dir
    if (mean is None) != (inv_std is None):
        raise _lib.SwimmerHipError("mean and inv_std must be given together")
    if traj is not None:
        _want(traj, "traj", (H, p.d, n_roll))
    if moments is not None:
        _want(moments, "moments", (moments_blocks(n_roll), 2 * p.d))
    returns = _f64((n_roll,), dev) if returns is None else _want(returns, "returns", (n_roll,))
    check(load().sw_ars_rollouts_f64(ctypes.byref(p), dir_begin, n_dir, H, ptr(policy),
                                     ptr(deltas), float(nu), ptr(mean), ptr(inv_std),
                                     ptr(returns), ptr(traj), ptr(moments), ptr(status),
                                     stream_ptr()), "sw_ars_rollouts_f64")
    return returns


def ars_gate(p_sim: SwParams, H: int, policy, deltas, nu: float, dir_begin: int, n_dir: int,
             sim_thresh: float, mean=None, inv_std=None, returns=None, status=None, admit=None):
    """The safe-ARS simulator gate (ars_agent.py:144-157): the 2*n_dir rollouts P +- nu*delta_i in the
    simulator p_sim and, in the same launch, admit[j] = !(r_j+ <= sim_thresh) && !(r_j- <= sim_thresh).
    Returns admit, an int32 device tensor [n_dir] (1 = take the real rollouts).  `returns` / `status`
    ([2*n_dir], optional) receive the simulator returns / status codes as ars_rollouts writes them; `admit`
    (optional) is an int32 [n_dir] tensor to write the flags into instead of a new one."""
    require_gpu()
    _want(policy, "policy", (p_sim.m, p_sim.d))
    if deltas.dim() != 3 or deltas.shape[0] < dir_begin + n_dir:
        raise _lib.SwimmerHipError("deltas: need [>= dir_begin + n_dir, m, d]")
    _want(deltas, "deltas", (deltas.shape[0], p_sim.m, p_sim.d))
    dev = policy.device
    n_roll = 2 * n_dir
    if (mean is None) != (inv_std is None):
        raise _lib.SwimmerHipError("mean and inv_std must be given together")
    if mean is not None:
        _want(mean, "mean", (p_sim.d,))
        _want(inv_std, "inv_std", (p_sim.d,))
    if returns is not None:
        _want(returns, "returns", (n_roll,))
    if status is not None and (status.dtype != torch.int32 or tuple(status.shape) != (n_roll,)
                               or status.device != dev):
        raise _lib.SwimmerHipError(f"status: expected int32 tensor of shape ({n_roll},) on {dev}")
    if admit is None:
        admit = torch.empty(n_dir, dtype=torch.int32, device=dev)
    elif admit.dtype != torch.int32 or tuple(admit.shape) != (n_dir,) or admit.device != dev:
        raise _lib.SwimmerHipError(f"admit: expected int32 tensor of shape ({n_dir},) on {dev}")
    check(load().sw_ars_gate_f64(ctypes.byref(p_sim), dir_begin, n_dir, H, ptr(policy), ptr(deltas),
                                 float(nu), ptr(mean), ptr(inv_std), float(sim_thresh), ptr(admit),
                                 ptr(returns), ptr(status), stream_ptr()), "sw_ars_gate_f64")
    return admit


def ars_update(p: SwParams, returns, deltas, policy, alpha: float, b: float, top_b: int = 0,
               moments=None, running=None, n_new_states: int = 0, mean=None, inv_std=None,
               sigma_out=None):
    """In-place ARS update of `policy` (+ V2 statistics when `running` is given)."""
    require_gpu()
    n_dir = returns.shape[0] // 2
    _want(returns, "returns", (2 * n_dir,))
    _want(policy, "policy", (p.m, p.d))
    _want(deltas, "deltas", (deltas.shape[0], p.m, p.d))
    if deltas.shape[0] < n_dir:
        raise _lib.SwimmerHipError("deltas: fewer directions than returns")
    n_rows = 0
    if running is not None:
        _want(running, "running", (1 + 2 * p.d,))
        _want(mean, "mean", (p.d,))
        _want(inv_std, "inv_std", (p.d,))
        n_rows = moments.shape[0]
        _want(moments, "moments", (n_rows, 2 * p.d))
    check(load().sw_ars_update_f64(ctypes.byref(p), n_dir, ptr(returns), ptr(deltas),
                                   ptr(policy), float(alpha), float(b), int(top_b),
                                   ptr(moments), n_rows, ptr(running), int(n_new_states),
                                   ptr(mean), ptr(inv_std), ptr(sigma_out), stream_ptr()),
          "sw_ars_update_f64")
    return policy


def _want_i32(t, name, shape, device):
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape) or t.device != device:
        raise _lib.SwimmerHipError(f"{name}: expected int32 tensor of shape {tuple(shape)} on {device}")
    return t


def ars_rollouts_multi(p: SwParams, H: int, policy, deltas, nu: float, mean=None, inv_std=None, returns=None,
                       moments=None, status=None):
    """The exploration rollouts of S agents in ONE launch (sw_ars_rollouts_multi_f64): policy [S, m, d], deltas
    [S, N, m, d], mean / inv_std [S, d] (both or neither).  Returns `returns` [S, 2N]: row a holds what
    ars_rollouts gives for agent a's policy, deltas, mean and inv_std; moments ([S, moments_blocks(2N), 2d]) and
    status (int32 [S, 2N]) are filled when given, agent by agent as ars_rollouts fills them."""
    require_gpu()
    if policy.dim() != 3 or policy.shape[0] < 1:
        raise _lib.SwimmerHipError(f"policy: expected float64 tensor of shape (S, m, d), got {tuple(policy.shape)}")
    S = policy.shape[0]
    _want(policy, "policy", (S, p.m, p.d))
    if deltas.dim() != 4 or deltas.shape[1] < 1:
        raise _lib.SwimmerHipError(f"deltas: expected float64 tensor of shape (S, N, m, d), got {tuple(deltas.shape)}")
    N = deltas.shape[1]
    _want(deltas, "deltas", (S, N, p.m, p.d))
    dev = policy.device
    if (mean is None) != (inv_std is None):
        raise _lib.SwimmerHipError("mean and inv_std must be given together")
    if mean is not None:
        _want(mean, "mean", (S, p.d))
        _want(inv_std, "inv_std", (S, p.d))
    if moments is not None:
        _want(moments, "moments", (S, moments_blocks(2 * N), 2 * p.d))
    if status is not None:
        _want_i32(status, "status", (S, 2 * N), dev)
    returns = _f64((S, 2 * N), dev) if returns is None else _want(returns, "returns", (S, 2 * N))
    check(load().sw_ars_rollouts_multi_f64(ctypes.byref(p), S, N, H, ptr(policy), ptr(deltas), float(nu), ptr(mean),
                                           ptr(inv_std), ptr(returns), ptr(moments), ptr(status), stream_ptr()),
          "sw_ars_rollouts_multi_f64")
    return returns


def ars_update_multi(p: SwParams, returns, deltas, policy, alpha: float, b: float, top_b: int = 0,
                     moments=None, running=None, n_new_states: int = 0, mean=None, inv_std=None,
                     sigma_out=None):
    """ars_update for S agents in ONE launch (sw_ars_update_multi_f64), in place: returns [S, 2N], deltas
    [S, N, m, d], policy [S, m, d]; with `running` ([S, 1 + 2d]) also moments [S, rows, 2d], mean and inv_std
    [S, d]; sigma_out [S] or None."""
    require_gpu()
    if returns.dim() != 2 or returns.shape[0] < 1 or returns.shape[1] < 2 or returns.shape[1] % 2:
        raise _lib.SwimmerHipError(f"returns: expected float64 tensor of shape (S, 2N), got {tuple(returns.shape)}")
    S, n_dir = returns.shape[0], returns.shape[1] // 2
    _want(returns, "returns", (S, 2 * n_dir))
    _want(policy, "policy", (S, p.m, p.d))
    _want(deltas, "deltas", (S, n_dir, p.m, p.d))
    n_rows = 0
    if running is not None:
        _want(running, "running", (S, 1 + 2 * p.d))
        _want(mean, "mean", (S, p.d))
        _want(inv_std, "inv_std", (S, p.d))
        if moments is None or moments.dim() != 3:
            raise _lib.SwimmerHipError("moments: expected float64 tensor of shape (S, rows, 2d) next to running")
        n_rows = moments.shape[1]
        _want(moments, "moments", (S, n_rows, 2 * p.d))
    if sigma_out is not None:
        _want(sigma_out, "sigma_out", (S,))
    check(load().sw_ars_update_multi_f64(ctypes.byref(p), S, n_dir, ptr(returns), ptr(deltas), ptr(policy),
                                         float(alpha), float(b), int(top_b), ptr(moments), n_rows, ptr(running),
                                         int(n_new_states), ptr(mean), ptr(inv_std), ptr(sigma_out), stream_ptr()),
          "sw_ars_update_multi_f64")
    return policy


def _multi_shapes(p, policy, deltas, mean, inv_std):
    """(S, N, device) of a multi-agent launch's policy [S, m, d] and deltas [S, N, m, d], checked with mean / inv_std."""
    if policy.dim() != 3 or policy.shape[0] < 1:
        raise _lib.SwimmerHipError(f"policy: expected float64 tensor of shape (S, m, d), got {tuple(policy.shape)}")
    S = policy.shape[0]
    _want(policy, "policy", (S, p.m, p.d))
    if deltas.dim() != 4 or deltas.shape[1] < 1:
        raise _lib.SwimmerHipError(f"deltas: expected float64 tensor of shape (S, N, m, d), got {tuple(deltas.shape)}")
    N = deltas.shape[1]
    _want(deltas, "deltas", (S, N, p.m, p.d))
    if (mean is None) != (inv_std is None):
        raise _lib.SwimmerHipError("mean and inv_std must be given together")
    if mean is not None:
        _want(mean, "mean", (S, p.d))
        _want(inv_std, "inv_std", (S, p.d))
    return S, N, policy.device


def ars_gate_multi(p_base: SwParams, H: int, policy, deltas, nu: float, sim, sim_thresh, mean=None, inv_std=None,
                   returns=None, status=None, admit=None):
    """ars_gate for S agents in ONE launch (sw_ars_gate_multi_f64), every agent in a simulator and against a threshold
    of its own: policy [S, m, d], deltas [S, N, m, d], sim [S, 3] = each agent's (l_i, m_i, k), sim_thresh [S];
    n, h, the direction and the flags of every simulator come from p_base.  Returns admit (int32 [S, N]); `returns`
    ([S, 2N]) and `status` (int32 [S, 2N]) receive the simulator returns and status codes, row a as ars_gate gives
    them for agent a.  A simulator that breaks the parameter rule: SW_STATUS_PARAM, nothing admitted."""
    require_gpu()
    S, N, dev = _multi_shapes(p_base, policy, deltas, mean, inv_std)
    _want(sim, "sim", (S, 3))
    _want(sim_thresh, "sim_thresh", (S,))
    returns = _f64((S, 2 * N), dev) if returns is None else _want(returns, "returns", (S, 2 * N))
    if status is not None:
        _want_i32(status, "status", (S, 2 * N), dev)
    admit = (torch.empty((S, N), dtype=torch.int32, device=dev) if admit is None
             else _want_i32(admit, "admit", (S, N), dev))
    check(load().sw_ars_gate_multi_f64(ctypes.byref(p_base), S, N, H, ptr(policy), ptr(deltas), float(nu), ptr(mean),
                                       ptr(inv_std), ptr(sim), ptr(sim_thresh), ptr(admit), ptr(returns),
                                       ptr(status), stream_ptr()), "sw_ars_gate_multi_f64")
    return admit


def ars_pack_admitted(p: SwParams, admit, deltas, status=None, count=None, order=None, packed=None):
    """The gate's flags into what the counted launches read (sw_ars_pack_admitted_f64): admit int32 [S, N] (and the
    gate's status int32 [S, 2N]: a direction with a failed simulator rollout counts as refused), deltas [S, N, m, d]
    -> (count int32 [S], order int32 [S, N]: the admitted indices ascending, then -1, packed [S, N, m, d]: their
    deltas in that order in entries 0..count-1; the entries behind them are not written)."""
    require_gpu()
    if admit.dim() != 2 or admit.shape[0] < 1 or admit.shape[1] < 1:
        raise _lib.SwimmerHipError(f"admit: expected int32 tensor of shape (S, N), got {tuple(admit.shape)}")
    S, N = admit.shape
    dev = deltas.device
    _want_i32(admit, "admit", (S, N), dev)
    _want(deltas, "deltas", (S, N, p.m, p.d))
    if status is not None:
        _want_i32(status, "status", (S, 2 * N), dev)
    count = torch.empty(S, dtype=torch.int32, device=dev) if count is None else _want_i32(count, "count", (S,), dev)
    order = (torch.empty((S, N), dtype=torch.int32, device=dev) if order is None
             else _want_i32(order, "order", (S, N), dev))
    packed = torch.zeros_like(deltas) if packed is None else _want(packed, "packed", (S, N, p.m, p.d))
    check(load().sw_ars_pack_admitted_f64(ctypes.byref(p), S, N, ptr(admit), ptr(status), ptr(deltas), ptr(count),
                                          ptr(order), ptr(packed), stream_ptr()), "sw_ars_pack_admitted_f64")
    return count, order, packed


def ars_rollouts_multi_counted(p: SwParams, H: int, policy, deltas, nu: float, count, mean=None, inv_std=None,
                               returns=None, moments=None, status=None):
    """ars_rollouts_multi with every agent's direction count read on the device (sw_ars_rollouts_multi_counted_f64):
    count int32 [S]; agent a runs the 2 count[a] rollouts of its first count[a] deltas and writes returns / status
    entries 0..2 count[a] - 1 and its first moments_blocks(2 count[a]) moment rows; everything behind is left as it
    was (a new `returns` starts as NaN).  N = deltas.shape[1] is the maximum and sets the strides."""
    require_gpu()
    S, N, dev = _multi_shapes(p, policy, deltas, mean, inv_std)
    _want_i32(count, "count", (S,), dev)
    if moments is not None:
        _want(moments, "moments", (S, moments_blocks(2 * N), 2 * p.d))
    if status is not None:
        _want_i32(status, "status", (S, 2 * N), dev)
    if returns is None:
        returns = torch.full((S, 2 * N), float("nan"), dtype=torch.float64, device=dev)
    else:
        _want(returns, "returns", (S, 2 * N))
    check(load().sw_ars_rollouts_multi_counted_f64(ctypes.byref(p), S, N, ptr(count), H, ptr(policy), ptr(deltas),
                                                   float(nu), ptr(mean), ptr(inv_std), ptr(returns), ptr(moments),
                                                   ptr(status), stream_ptr()), "sw_ars_rollouts_multi_counted_f64")
    return returns


def ars_update_multi_counted(p: SwParams, H: int, count, returns, deltas, policy, alpha: float, b: float,
                             top_b: int = 0, moments=None, running=None, mean=None, inv_std=None, sigma_out=None):
    """ars_update_multi with per-agent n_dir = count[a], top_b = min(top_b, count[a]) and n_new_states =
    2 count[a] H (sw_ars_update_multi_counted_f64), in place; an agent with count 0 is left untouched.  Shapes as
    ars_update_multi with N the maximum; moments [S, rows >= moments_blocks(2N), 2d]."""
    require_gpu()
    if returns.dim() != 2 or returns.shape[0] < 1 or returns.shape[1] < 2 or returns.shape[1] % 2:
        raise _lib.SwimmerHipError(f"returns: expected float64 tensor of shape (S, 2N), got {tuple(returns.shape)}")
    S, n_dir = returns.shape[0], returns.shape[1] // 2
    _want(returns, "returns", (S, 2 * n_dir))
    _want(policy, "policy", (S, p.m, p.d))
    _want(deltas, "deltas", (S, n_dir, p.m, p.d))
    _want_i32(count, "count", (S,), policy.device)
    n_rows = 0
    if running is not None:
        _want(running, "running", (S, 1 + 2 * p.d))
        _want(mean, "mean", (S, p.d))
        _want(inv_std, "inv_std", (S, p.d))
        if moments is None or moments.dim() != 3 or moments.shape[1] < moments_blocks(2 * n_dir):
            raise _lib.SwimmerHipError("moments: expected float64 tensor of shape (S, rows >= moments_blocks(2N), 2d) "
                                       "next to running")
        n_rows = moments.shape[1]
        _want(moments, "moments", (S, n_rows, 2 * p.d))
    if sigma_out is not None:
        _want(sigma_out, "sigma_out", (S,))
    check(load().sw_ars_update_multi_counted_f64(ctypes.byref(p), S, n_dir, ptr(count), H, ptr(returns), ptr(deltas),
                                                 ptr(policy), float(alpha), float(b), int(top_b), ptr(moments), n_rows,
                                                 ptr(running), ptr(mean), ptr(inv_std), ptr(sigma_out), stream_ptr()),
          "sw_ars_update_multi_counted_f64")
    return policy


def safe_ars_rollouts_multi(p_real: SwParams, H: int, policy, deltas, nu: float, gated, sim, sim_thresh, real_thresh,
                            cost_kind: int, cost_index: int, returns=None, cost_trace=None, cost_max=None,
                            first_refused=None, violations=None, status=None):
    """The exploration rollouts of A Basic_ARS / Safe_ARS agents in ONE launch (sw_safe_ars_rollouts_multi_f64):
    policy [A, m, d], deltas [A, N, m, d], gated int32 [A] (0: every step is taken; else the per-step simulator gate),
    sim [A, 3] = each agent's simulator (l_i, m_i, k), sim_thresh / real_thresh [A].  Returns `returns` [A, 2N]: row a
    holds what safe_rollouts (gated) or rollout (ungated) gives for agent a's policies P + / - nu delta.  Optional
    outputs, filled when given: cost_trace [H, A, 2N] (the cost of the state after step t, of the unchanged state where
    the step was refused), cost_max [A, 2N], first_refused / violations / status int32 [A, 2N].  A gated agent whose
    simulator breaks the parameter rule: SW_STATUS_PARAM, NaN returns, first_refused 0."""
    require_gpu()
    A, N, dev = _multi_shapes(p_real, policy, deltas, None, None)
    _want_i32(gated, "gated", (A,), dev)
    _want(sim, "sim", (A, 3))
    _want(sim_thresh, "sim_thresh", (A,))
    _want(real_thresh, "real_thresh", (A,))
    if cost_trace is not None:
        _want(cost_trace, "cost_trace", (H, A, 2 * N))
    if cost_max is not None:
        _want(cost_max, "cost_max", (A, 2 * N))
    for name, t in (("first_refused", first_refused), ("violations", violations), ("status", status)):
        if t is not None:
            _want_i32(t, name, (A, 2 * N), dev)
    returns = _f64((A, 2 * N), dev) if returns is None else _want(returns, "returns", (A, 2 * N))
    check(load().sw_safe_ars_rollouts_multi_f64(ctypes.byref(p_real), A, N, H, ptr(policy), ptr(deltas), float(nu),
                                                ptr(gated), ptr(sim), ptr(sim_thresh), ptr(real_thresh),
                                                int(cost_kind), int(cost_index), ptr(returns), ptr(cost_trace),
                                                ptr(cost_max), ptr(first_refused), ptr(violations), ptr(status),
                                                stream_ptr()), "sw_safe_ars_rollouts_multi_f64")
    return returns


CACLA_HIDDEN = 12   # SW_CACLA_HIDDEN: the reference's hidden width (cacla_agent.py:165-166)


def cacla_net_doubles(n: int) -> int:
    """SW_CACLA_NET_DOUBLES(n): one TwoLayersNet(d = 2n + 2, 12) as W1 [12][d] | b1 [12] | W2 [12] | b2."""
    return CACLA_HIDDEN * (2 * n + 2) + 2 * CACLA_HIDDEN + 1


def cacla_run(p: SwParams, n_iter: int, train: bool, gamma, alpha, noise, weights, state, rewards=None,
              actor_updates=None, status=None):
    """n_iter CACLA steps of A independent agents in ONE launch (sw_cacla_run_f64), one wave per agent: gamma, alpha
    [A], noise [A, n_iter, m] (added to the actors' outputs), weights [A, n, cacla_net_doubles(n)] and state [A, d]
    updated in place (weights only when training), actor_updates / status int32 [A] accumulated when given.
    Returns `rewards` [A, n_iter]."""
    require_gpu()
    if gamma.dim() != 1 or gamma.shape[0] < 1:
        raise _lib.SwimmerHipError(f"gamma: expected float64 tensor of shape (A,), got {tuple(gamma.shape)}")
    A, dev = gamma.shape[0], gamma.device
    _want(gamma, "gamma", (A,))
    _want(alpha, "alpha", (A,))
    _want(noise, "noise", (A, n_iter, p.m))
    _want(weights, "weights", (A, p.n, cacla_net_doubles(p.n)))
    _want(state, "state", (A, p.d))
    if actor_updates is not None:
        _want_i32(actor_updates, "actor_updates", (A,), dev)
    if status is not None:
        _want_i32(status, "status", (A,), dev)
    rewards = _f64((A, n_iter), dev) if rewards is None else _want(rewards, "rewards", (A, n_iter))
    check(load().sw_cacla_run_f64(ctypes.byref(p), A, int(n_iter), 1 if train else 0, ptr(gamma), ptr(alpha),
                                  ptr(noise), ptr(weights), ptr(state), ptr(rewards), ptr(actor_updates),
                                  ptr(status), stream_ptr()), "sw_cacla_run_f64")
    return rewards


def ars_update_gathered(p: SwParams, n_dir: int, gathered, world: int, chunk: int, rows_chunk: int,
                        deltas, policy, alpha: float, b: float, top_b: int = 0, running=None,
                        n_new_states: int = 0, mean=None, inv_std=None, sigma_out=None):
    """The ARS update reading the all-gathered result segments in place: `gathered` holds
    `world` segments [2*chunk returns | rows_chunk moment rows of 2d] (sw_ars_update_gathered_f64)."""
    require_gpu()
    seg = 2 * chunk + rows_chunk * 2 * p.d
    _want(gathered, "gathered", (world * seg,))
    _want(policy, "policy", (p.m, p.d))
    _want(deltas, "deltas", (deltas.shape[0], p.m, p.d))
    if deltas.shape[0] < n_dir:
        raise _lib.SwimmerHipError("deltas: fewer directions than n_dir")
    if running is not None:
        _want(running, "running", (1 + 2 * p.d,))
        _want(mean, "mean", (p.d,))
        _want(inv_std, "inv_std", (p.d,))
    check(load().sw_ars_update_gathered_f64(
        ctypes.byref(p), int(n_dir), ptr(gathered), int(world), int(chunk), int(rows_chunk),
        ptr(deltas), ptr(policy), float(alpha), float(b), int(top_b), ptr(running),
        int(n_new_states), ptr(mean), ptr(inv_std), ptr(sigma_out), stream_ptr()),
        "sw_ars_update_gathered_f64")
    return policy


def issue_interval_ns(mode: int, device="cuda:0", trips: int = 8192):
    """Lone-wave issue interval of one instruction class on this device (mode 0: independent
    v_fma_f64, 1: v_mov_b32): HIP events around sw_issue_probe, nanoseconds per instruction."""
    require_gpu()
    scratch = torch.empty(64, dtype=torch.float64, device=device)
    fn = load().sw_issue_probe
    best = None
    for _ in range(3):
        check(fn(mode, 16, ptr(scratch), stream_ptr()), "sw_issue_probe")      # warm
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        check(fn(mode, trips, ptr(scratch), stream_ptr()), "sw_issue_probe")
        e1.record()
        check(fn(mode, 2 * trips, ptr(scratch), stream_ptr()), "sw_issue_probe")
        e2.record()
        torch.cuda.synchronize()
        # the difference of the two launches cancels the fixed launch cost
        ns = (e1.elapsed_time(e2) - e0.elapsed_time(e1)) * 1e6 / (trips * 64)
        best = ns if best is None else min(best, ns)
    return best


def issue_interval_full_chip_ns(mode: int, device="cuda:0", trips: int = 8192, workgroups: int = 256, waves: int = 4,
                                settle_ms: float = 60.0):
    """The same interval with a wave on EVERY SIMD (sw_issue_probe_grid, 256 workgroups x 4 waves): what an
    instruction costs a wave once the whole chip issues -- f64 on every SIMD lowers the clock the chip
    sustains, so the probe first loads the chip for `settle_ms` and then reports the MEDIAN of five
    difference measurements (the lone-wave probe reports the best of three)."""
    require_gpu()
    scratch = torch.empty(64, dtype=torch.float64, device=device)
    fn = load().sw_issue_probe_grid

    def go(t):
        check(fn(mode, t, workgroups, waves, ptr(scratch), stream_ptr()), "sw_issue_probe_grid")
    per_launch_ms = trips * 64 * 2.3e-6
    for _ in range(max(1, int(settle_ms / per_launch_ms))):
        go(trips)
    samples = []
    for _ in range(5):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        go(trips)
        e1.record()
        go(2 * trips)
        e2.record()
        torch.cuda.synchronize()
        samples.append((e1.elapsed_time(e2) - e0.elapsed_time(e1)) * 1e6 / (trips * 64))
    return sorted(samples)[2]


def cov_acc_doubles(p: SwParams, n_roll: int, H: int) -> int:
    """Doubles in the accumulator of a covariance pass over (n_roll, H): the 1 + d + d*d sums
    followed by the pass's scratch (include/swimmer_hip.h)."""
    n = int(load().sw_cov_acc_doubles(ctypes.byref(p), int(n_roll), int(H)))
    if n < 0:
        raise _lib.SwimmerHipError("sw_cov_acc_doubles: bad arguments")
    return n


def new_cov_acc(p: SwParams, n_roll: int, H: int, device):
    return torch.zeros(cov_acc_doubles(p, n_roll, H), dtype=torch.float64, device=device)


def traj_moments(p: SwParams, traj, acc=None):
    """acc[:1 + d + d*d] += {count, sum(s-c), sum((s-c)(s-c)^T)} over traj [H, d, n_roll];
    acc = new_cov_acc(p, n_roll, H, device) (sums + scratch), reusable for further passes of
    the same shape.  Deterministic (no floating-point atomics)."""
    require_gpu()
    H, d, n_roll = traj.shape
    _want(traj, "traj", (H, p.d, n_roll))
    if acc is None:
        acc = new_cov_acc(p, n_roll, H, traj.device)
    if acc.dtype != torch.float64 or acc.dim() != 1 or acc.numel() < cov_acc_doubles(p, n_roll, H):
        raise _lib.SwimmerHipError("acc: need a float64 vector of cov_acc_doubles(p, n_roll, H)")
    check(load().sw_traj_moments_f64(ctypes.byref(p), n_roll, H, ptr(traj), ptr(acc),
                                     stream_ptr()), "sw_traj_moments_f64")
    return acc


class ArsPipeline(object):
    """Handle of a native sw_ars_pipeline (include/swimmer_hip.h): the ring-buffered
    copy stream + progress flag + ride-along covariance schedule of one ARS iteration,
    enqueued from C."""

    def __init__(self):
        require_gpu()
        h = ctypes.c_void_p()
        check(load().sw_ars_pipeline_create(ctypes.byref(h)), "sw_ars_pipeline_create")
        self._h = h
        self.slots = int(load().sw_ars_pipeline_slots())

    def close(self):
        if getattr(self, "_h", None) is not None:
            load().sw_ars_pipeline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def next_slot(self):
        """Ring slot of the next rollouts() call (the pipeline's own call count mod slots)."""
        return int(load().sw_ars_pipeline_next_slot(self._h))

    def host_slot_wait(self, slot):
        check(load().sw_ars_pipeline_host_slot_wait(self._h, slot), "sw_ars_pipeline_host_slot_wait")

    def sync_cov(self):
        check(load().sw_ars_pipeline_sync_cov(self._h), "sw_ars_pipeline_sync_cov")

    def timing(self, every):
        """every = k > 0: HIP events around every k-th rollout launch; 0 / False: off."""
        check(load().sw_ars_pipeline_timing(self._h, int(every)), "sw_ars_pipeline_timing")

    def rollout_ms(self):
        ms, n = ctypes.c_double(), ctypes.c_int64()
        check(load().sw_ars_pipeline_rollout_ms(self._h, ctypes.byref(ms), ctypes.byref(n)),
              "sw_ars_pipeline_rollout_ms")
        return ms.value, n.value

    def rollouts(self, slot, p, n_dir_total, dir_begin, n_dir, H, deltas_host, deltas_dev, policy,
                 nu, mean, inv_std, returns, traj, moments, cov_acc, status):
        """deltas_host: pinned CPU tensor [n_dir_total, m, d]; everything else on the GPU."""
        if not deltas_host.is_pinned() or not deltas_host.is_contiguous():
            raise _lib.SwimmerHipError("deltas_host must be a contiguous pinned CPU tensor")
        check(load().sw_ars_iteration_rollouts_f64(
            self._h, slot, ctypes.byref(p), n_dir_total, dir_begin, n_dir, H,
            ctypes.c_void_p(deltas_host.data_ptr()), ptr(deltas_dev), ptr(policy), float(nu),
            ptr(mean), ptr(inv_std), ptr(returns), ptr(traj), ptr(moments), ptr(cov_acc),
            ptr(status), stream_ptr()), "sw_ars_iteration_rollouts_f64")

    def update(self, slot, p, n_dir, gathered, world, chunk, rows_chunk, deltas_dev, policy,
               alpha, b, top_b, running, n_new_states, mean, inv_std, sigma_out):
        """gathered: [world * (2*chunk + rows_chunk*2d)] all-gathered segments (see
        sw_ars_update_gathered_f64); world = 1: this rank's own segment."""
        check(load().sw_ars_iteration_update_f64(
            self._h, slot, ctypes.byref(p), n_dir, ptr(gathered), int(world), int(chunk),
            int(rows_chunk), ptr(deltas_dev), ptr(policy), float(alpha), float(b), int(top_b),
            ptr(running), int(n_new_states), ptr(mean), ptr(inv_std), ptr(sigma_out),
            stream_ptr()), "sw_ars_iteration_update_f64")


LQR_MAX_STATE, LQR_MAX_ACTION = 4, 2                       # SW_LQR_MAX_STATE, SW_LQR_MAX_ACTION
LQR_THRESHOLD_STEP, LQR_THRESHOLD_FIXED = 0, 1             # SW_LQR_THRESHOLD_*
LQR_COST_INF, LQR_COST_2, LQR_COST_1 = 0, 1, 2             # SW_LQR_COST_*
LQR_REFUSED, LQR_ADMITTED, LQR_NOTHING_YET = 0, 1, 2       # SW_LQR_REFUSED / ADMITTED / NOTHING_YET


def lqr_model_doubles(ns: int, na: int) -> int:
    """SW_LQR_MODEL_DOUBLES: A [ns][ns] | B [ns][na] | C [ns] | max_s | max_a."""
    return ns * ns + ns * na + ns + 2


def lqr_param_doubles(ns: int, na: int) -> int:
    """SW_LQR_PARAM_DOUBLES: real model | simulator model | Q | R | gamma alpha l eps_Lc dA dB fixed threshold."""
    return 2 * lqr_model_doubles(ns, na) + ns * ns + na * na + 7


def lqr_cacla_run(ns: int, na: int, n_iter: int, safe: bool, threshold: int, cost: int, params, noise, F, V, state,
                  last, counters, status, rec_state=None, rec_action=None, rec_reward=None, rec_admitted=None):
    """n_iter steps of CACLA on LQR for A independent agents in ONE launch (sw_lqr_cacla_run_f64), one agent per lane.
    Every tensor is agent-minor: params [lqr_param_doubles, A], noise [n_iter, na, A], F [na, ns, A], V and state
    [ns, A], last [ns + na + 1, A], counters int32 [3, A] (admitted, violations, actor_updates) and status int32 [A]
    are updated in place; the records rec_state [n_iter, ns, A], rec_action [n_iter, na, A], rec_reward [n_iter, A]
    and rec_admitted uint8 [n_iter, A] are written when given."""
    require_gpu()
    if params.dim() != 2 or params.shape[1] < 1:
        raise _lib.SwimmerHipError(f"params: expected float64 tensor of shape (P, A), got {tuple(params.shape)}")
    A, dev = params.shape[1], params.device
    _want(params, "params", (lqr_param_doubles(ns, na), A))
    _want(noise, "noise", (n_iter, na, A))
    _want(F, "F", (na, ns, A))
    _want(V, "V", (ns, A))
    _want(state, "state", (ns, A))
    _want(last, "last", (ns + na + 1, A))
    _want_i32(counters, "counters", (3, A), dev)
    _want_i32(status, "status", (A,), dev)
    for t, name, shape in ((rec_state, "rec_state", (n_iter, ns, A)), (rec_action, "rec_action", (n_iter, na, A)),
                           (rec_reward, "rec_reward", (n_iter, A))):
        if t is not None:
            _want(t, name, shape)
    if rec_admitted is not None and (rec_admitted.dtype != torch.uint8 or tuple(rec_admitted.shape) != (n_iter, A)):
        raise _lib.SwimmerHipError(f"rec_admitted: expected uint8 tensor of shape {(n_iter, A)}")
    check(load().sw_lqr_cacla_run_f64(int(ns), int(na), A, int(n_iter), 1 if safe else 0, int(threshold), int(cost),
                                      ptr(params), ptr(noise), ptr(F), ptr(V), ptr(state), ptr(last), ptr(counters),
                                      ptr(status), ptr(rec_state), ptr(rec_action), ptr(rec_reward),
                                      ptr(rec_admitted), stream_ptr()), "sw_lqr_cacla_run_f64")
