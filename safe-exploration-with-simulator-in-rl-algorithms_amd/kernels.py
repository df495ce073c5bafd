"""Functional wrappers: torch device tensors in, one C-ABI call (include/swimmer_hip.h) each.

Shapes follow the ABI: states are SoA [d, n_env], actions [m, n_env], policies AoS
[n_roll, m, d], trajectories [H, d, n_roll].  Everything is float64 and stays on the GPU;
all calls are asynchronous on torch's current stream.

Every tensor a wrapper hands to the library goes through ONE check first (`_tensor`, with `_opt` for an argument that
may be None and `_out` for an output that is allocated when None): dtype, exact shape (or a lower bound where the ABI
has one), contiguity, and the device of the call's first required tensor, which must be a GPU.  A miss is a
SwimmerHipError that names the parameter, what was expected and what was given, before anything is launched.  The
one exception are the pre-bound hot paths, whose buffers are their owner's, allocated once: StepPlan.launch (its
constructor checks, once), SingleEnv (no tensors at all) and ArsPipeline.rollouts / ArsPipeline.update.
"""
import ctypes

import torch

from . import _lib
from ._lib import SwParams, SwimmerHipError, check, load, ptr, require_gpu, stream_ptr

_I32 = torch.int32


class _Min(int):
    """A shape entry that is a lower bound on the size, not the size."""

    def __repr__(self):
        return f">={int(self)}"


_ANY = _Min(0)


def _describe(t):
    if not isinstance(t, torch.Tensor):
        return "None" if t is None else type(t).__name__
    return f"{t.dtype} {tuple(t.shape)} on {t.device}" + ("" if t.is_contiguous() else ", not contiguous")


def _tensor(t, name, shape, on, dtype=torch.float64):
    """The argument check of every wrapper: `t` is a contiguous `dtype` tensor of `shape` (a tuple; _Min entries are
    lower bounds) on the call's device: `on` = (device, the parameter that set it).  -> t, or SwimmerHipError."""
    if (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == on[0] and t.is_contiguous()
            and (t.shape == shape or (len(t.shape) == len(shape) and all(
                g >= w if isinstance(w, _Min) else g == w for g, w in zip(t.shape, shape))))):
        return t
    raise SwimmerHipError(f"{name}: expected a contiguous {dtype} tensor of shape {shape} on {on[0]} "
                          f"as {on[1]}, got {_describe(t)}")


def _opt(t, name, shape, on, dtype=torch.float64):
    """_tensor for an argument that may be None."""
    return None if t is None else _tensor(t, name, shape, on, dtype)


def _out(t, name, shape, on, dtype=torch.float64, fill=None):
    """_tensor for an output; None: a new tensor, uninitialised or filled with `fill`."""
    if t is not None:
        return _tensor(t, name, shape, on, dtype)
    if fill is None:
        return torch.empty(shape, dtype=dtype, device=on[0])
    return torch.full(shape, fill, dtype=dtype, device=on[0])


def _gpu(t, name, ndim):
    """The `on` of a call whose first required tensor is `t` ([ndim]-dimensional, so that the call's sizes can be
    read off it before its own check): its device, which must be a GPU."""
    device = t.device if isinstance(t, torch.Tensor) else None
    if device is None or device.type != "cuda" or t.dim() != ndim:
        raise SwimmerHipError(f"{name}: expected a {ndim}-D tensor on the GPU, got {_describe(t)}")
    return device, name


def _pair(mean, inv_std, shape, on, required=False):
    """mean and inv_std: both or neither (both when `required`)."""
    need = _tensor if required or mean is not None or inv_std is not None else _opt
    need(mean, "mean", shape, on)
    need(inv_std, "inv_std", shape, on)


def _transitions(p, state, action, *next_ref):
    """(d, T, on) of the SoA columns state [d, T], action [m, T] and, where there is one, next_ref [d, T]."""
    on = _gpu(state, "state", 2)
    d, T = p.d, state.shape[1]
    _tensor(state, "state", (d, T), on)
    _tensor(action, "action", (p.m, T), on)
    for t in next_ref:
        _tensor(t, "next_ref", (d, T), on)
    return d, T, on


def reset(p: SwParams, n_env: int, device="cuda:0", out=None):
    """SwimmerEnv.reset for n_env swimmers -> state [d, n_env]."""
    require_gpu()
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    state = _out(out, "out", (p.d, n_env), (device, "device"))
    check(load().sw_reset_f64(ctypes.byref(p), n_env, ptr(state), stream_ptr()), "sw_reset_f64")
    return state


def step(p: SwParams, state, action, out=None, reward=None, status=None):
    """One physics step.  Returns (next_state [d, n_env], reward [n_env])."""
    require_gpu()
    d, n_env, on = _transitions(p, state, action)
    out = _out(out, "out", (d, n_env), on)
    reward = _out(reward, "reward", (n_env,), on)
    _opt(status, "status", (n_env,), on, _I32)
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
    _, T, on = _transitions(p, state, action, next_ref)
    partial = _out(partial, "partial", (step_residual_blocks(T),), on)
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
    _, T, on = _transitions(p_base, state, action, next_ref)
    n_cand = _tensor(cand, "cand", (_Min(1), 3), on).shape[0]
    partial = _out(partial, "partial", (n_cand, step_residual_blocks(T)), on)
    value = _out(value, "value", (n_cand,), on, fill=0.0)   # zeros: with T = 0 the library writes nothing and I is 0
    status = _out(status, "status", (n_cand,), on, _I32, fill=0)
    check(load().sw_step_residual_pop_f64(ctypes.byref(p_base), n_cand, ptr(cand), T, ptr(state), ptr(action),
                                          ptr(next_ref), ptr(partial), ptr(value), ptr(status), stream_ptr()),
          "sw_step_residual_pop_f64")
    return value, partial, status


def _sets_shapes(p_base, set_begin, max_set_len, state, action, next_ref):
    """(T, n_set, blocks of the longest set, on) of transitions cut into sets by set_begin (int64 [n_set + 1])."""
    _, T, on = _transitions(p_base, state, action, next_ref)
    n_set = _tensor(set_begin, "set_begin", (_Min(2),), on, torch.int64).shape[0] - 1
    return T, n_set, step_residual_blocks(max_set_len), on


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
    T, n_set, nb, on = _sets_shapes(p_base, set_begin, max_set_len, state, action, next_ref)
    n_cand = _tensor(cand, "cand", (_Min(1), 3), on).shape[0]
    _tensor(cand_set, "cand_set", (n_cand,), on, _I32)
    partial = _out(partial, "partial", (n_cand, nb), on)
    value = _out(value, "value", (n_cand,), on)
    status = _out(status, "status", (n_cand,), on, _I32, fill=0)
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
    T, n_set, nb, on = _sets_shapes(p_base, set_begin, max_set_len, state, action, next_ref)
    n_point = _tensor(points, "points", (n_set, _ANY, 3), on).shape[1]
    K = 13 if n_point == 7 else 1
    _opt(inv_2e, "inv_2e", (n_set, 3), on)
    _opt(active, "active", (n_set,), on, _I32)
    partial = _out(partial, "partial", (n_set, K, nb), on)
    out = _out(out, "out", (n_set, K), on)
    status = _out(status, "status", (n_set,), on, _I32, fill=0)
    check(load().sw_step_residual_normal_sets_f64(ctypes.byref(p_base), n_set, ptr(set_begin), int(max_set_len),
                                                  n_point, ptr(points), ptr(inv_2e), ptr(active), T, ptr(state),
                                                  ptr(action), ptr(next_ref), ptr(partial), ptr(out), ptr(status),
                                                  stream_ptr()), "sw_step_residual_normal_sets_f64")
    return out, status


class StepPlan(object):
    """A pre-bound sw_step_f64 launch: all argument conversion is done once, `launch()` is a
    single foreign call (the per-launch Python overhead of `step()` is larger than the 8192-env
    kernel itself).  Launches on the stream that was current when the plan was made.  The constructor checks the
    tensors as step() does, once; launch() checks nothing."""

    def __init__(self, p: SwParams, state, action, out, reward=None, status=None):
        require_gpu()
        d, n_env, on = _transitions(p, state, action)
        _tensor(out, "out", (d, n_env), on)
        _opt(reward, "reward", (n_env,), on)
        _opt(status, "status", (n_env,), on, _I32)
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
            raise SwimmerHipError("direct RCCL set-up failed on " +
                                  (f"this rank: {why}" if why else "another rank"))
        ident = broadcast_id(bytes(buf) if rank == 0 else None)
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(ident)
        h = ctypes.c_void_p()
        rc = lib.sw_comm_create(ctypes.byref(h), buf, world, rank)
        if not agree(rc == 0):
            if rc == 0:
                lib.sw_comm_destroy(h)
            raise SwimmerHipError("sw_comm_create failed on " +
                                  (f"this rank: {_lib.ERR_NAMES.get(rc, rc)}" if rc else "another rank"))
        self._h, self._lib, self.world, self.rank = h, lib, world, rank
        self._fn = lib.sw_comm_all_gather_f64

    def all_gather(self, send, gathered):
        """gathered[r * L : (r + 1) * L] <- rank r's send (L = send.numel()), on the current stream."""
        on = _gpu(send, "send", 1)
        L = _tensor(send, "send", (_ANY,), on).shape[0]
        _tensor(gathered, "gathered", (self.world * L,), on)
        rc = self._fn(self._h, ptr(send), ptr(gathered), L, stream_ptr())
        if rc:
            raise SwimmerHipError("sw_comm_all_gather_f64: " + self._lib.sw_comm_last_error(self._h).decode())
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
    one kernel launch and one host wait: no tensor is created, nothing is copied by a call, and there is no
    tensor argument to check."""
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
    _, n_env, on = _transitions(p, state, action)
    gdd = _out(None, "gdd", (2, n_env), on)
    tdd = _out(None, "tdd", (p.n, n_env), on)
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
    on = _gpu(policies, "policies", 3)
    n_roll = _tensor(policies, "policies", (_ANY, p.m, p.d), on).shape[0]
    _pair(mean, inv_std, (p.d,), on)
    _opt(state0, "state0", (p.d, n_roll), on)
    _opt(traj, "traj", (H, p.d, n_roll), on)
    _opt(final_state, "final_state", (p.d, n_roll), on)
    if moments is not None:
        _tensor(moments, "moments", (moments_blocks(n_roll), 2 * p.d), on)
    _opt(status, "status", (n_roll,), on, _I32)
    returns = _out(returns, "returns", (n_roll,), on)
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
    on = _gpu(policies, "policies", 3)
    n_roll = _tensor(policies, "policies", (_ANY, p_real.m, p_real.d), on).shape[0]
    _opt(traj, "traj", (H, p_real.d, n_roll), on)
    for name, t in (("first_refused", first_refused), ("violations", violations), ("status", status)):
        _opt(t, name, (n_roll,), on, _I32)
    returns = _out(returns, "returns", (n_roll,), on)
    check(load().sw_safe_rollouts_f64(ctypes.byref(p_real), ctypes.byref(p_sim), n_roll, H, ptr(policies),
                                      int(cost_kind), int(cost_index), float(sim_thresh), float(real_thresh),
                                      ptr(returns), ptr(traj), ptr(first_refused), ptr(violations), ptr(status),
                                      stream_ptr()), "sw_safe_rollouts_f64")
    return returns


def _ars_shapes(p, policy, deltas, dir_begin, n_dir, mean, inv_std):
    """(n_roll, on) of the 2 n_dir rollouts of policy [m, d] along deltas [>= dir_begin + n_dir, m, d], checked with
    mean / inv_std [d]."""
    on = _gpu(policy, "policy", 2)
    _tensor(policy, "policy", (p.m, p.d), on)
    _tensor(deltas, "deltas", (_Min(dir_begin + n_dir), p.m, p.d), on)
    _pair(mean, inv_std, (p.d,), on)
    return 2 * n_dir, on


def ars_rollouts(p: SwParams, H: int, policy, deltas, nu: float, dir_begin: int, n_dir: int,
                 mean=None, inv_std=None, returns=None, traj=None, moments=None, status=None):
    """The 2*n_dir exploration rollouts P +- nu*delta_i, i in [dir_begin, dir_begin+n_dir)."""
    require_gpu()
    n_roll, on = _ars_shapes(p, policy, deltas, dir_begin, n_dir, mean, inv_std)
    _opt(traj, "traj", (H, p.d, n_roll), on)
    if moments is not None:
        _tensor(moments, "moments", (moments_blocks(n_roll), 2 * p.d), on)
    _opt(status, "status", (n_roll,), on, _I32)
    returns = _out(returns, "returns", (n_roll,), on)
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
    n_roll, on = _ars_shapes(p_sim, policy, deltas, dir_begin, n_dir, mean, inv_std)
    _opt(returns, "returns", (n_roll,), on)
    _opt(status, "status", (n_roll,), on, _I32)
    admit = _out(admit, "admit", (n_dir,), on, _I32)
    check(load().sw_ars_gate_f64(ctypes.byref(p_sim), dir_begin, n_dir, H, ptr(policy), ptr(deltas),
                                 float(nu), ptr(mean), ptr(inv_std), float(sim_thresh), ptr(admit),
                                 ptr(returns), ptr(status), stream_ptr()), "sw_ars_gate_f64")
    return admit


def _update_state(p, lead, on, policy, running, mean, inv_std, sigma_out):
    """The tensors an ARS update changes, behind the agent dimensions `lead` (() for one agent): policy; running,
    with mean and inv_std required next to it; sigma_out."""
    _tensor(policy, "policy", lead + (p.m, p.d), on)
    _opt(running, "running", lead + (1 + 2 * p.d,), on)
    _pair(mean, inv_std, lead + (p.d,), on, required=running is not None)
    _opt(sigma_out, "sigma_out", lead or (1,), on)


def _update_moments(p, lead, on, moments, running, min_rows=0):
    """moments [rows >= min_rows, 2d] behind `lead`, required next to running -> the rows the update reads (none
    without running)."""
    if running is None:
        _opt(moments, "moments", lead + (_ANY, 2 * p.d), on)
        return 0
    return _tensor(moments, "moments", lead + (_Min(min_rows), 2 * p.d), on).shape[-2]


def _update_shapes(p, on, n_dir, deltas, policy, running, mean, inv_std, sigma_out):
    """The single-agent update's tensors behind its returns: deltas [>= n_dir, m, d] and _update_state's."""
    _tensor(deltas, "deltas", (_Min(n_dir), p.m, p.d), on)
    _update_state(p, (), on, policy, running, mean, inv_std, sigma_out)


def ars_update(p: SwParams, returns, deltas, policy, alpha: float, b: float, top_b: int = 0,
               moments=None, running=None, n_new_states: int = 0, mean=None, inv_std=None,
               sigma_out=None):
    """In-place ARS update of `policy` (+ V2 statistics when `running` is given)."""
    require_gpu()
    on = _gpu(returns, "returns", 1)
    n_dir = returns.numel() // 2
    _tensor(returns, "returns", (2 * n_dir,), on)
    _update_shapes(p, on, n_dir, deltas, policy, running, mean, inv_std, sigma_out)
    n_rows = _update_moments(p, (), on, moments, running)
    check(load().sw_ars_update_f64(ctypes.byref(p), n_dir, ptr(returns), ptr(deltas),
                                   ptr(policy), float(alpha), float(b), int(top_b),
                                   ptr(moments), n_rows, ptr(running), int(n_new_states),
                                   ptr(mean), ptr(inv_std), ptr(sigma_out), stream_ptr()),
          "sw_ars_update_f64")
    return policy


def _multi_shapes(p, policy, deltas, mean, inv_std):
    """(S, N, on) of a multi-agent launch's policy [S, m, d] and deltas [S, N, m, d], checked with mean / inv_std."""
    on = _gpu(policy, "policy", 3)
    S = _tensor(policy, "policy", (_Min(1), p.m, p.d), on).shape[0]
    N = _tensor(deltas, "deltas", (S, _Min(1), p.m, p.d), on).shape[1]
    _pair(mean, inv_std, (S, p.d), on)
    return S, N, on


def ars_rollouts_multi(p: SwParams, H: int, policy, deltas, nu: float, mean=None, inv_std=None, returns=None,
                       moments=None, status=None):
    """The exploration rollouts of S agents in ONE launch (sw_ars_rollouts_multi_f64): policy [S, m, d], deltas
    [S, N, m, d], mean / inv_std [S, d] (both or neither).  Returns `returns` [S, 2N]: row a holds what
    ars_rollouts gives for agent a's policy, deltas, mean and inv_std; moments ([S, moments_blocks(2N), 2d]) and
    status (int32 [S, 2N]) are filled when given, agent by agent as ars_rollouts fills them."""
    require_gpu()
    S, N, on = _multi_shapes(p, policy, deltas, mean, inv_std)
    if moments is not None:
        _tensor(moments, "moments", (S, moments_blocks(2 * N), 2 * p.d), on)
    _opt(status, "status", (S, 2 * N), on, _I32)
    returns = _out(returns, "returns", (S, 2 * N), on)
    check(load().sw_ars_rollouts_multi_f64(ctypes.byref(p), S, N, H, ptr(policy), ptr(deltas), float(nu), ptr(mean),
                                           ptr(inv_std), ptr(returns), ptr(moments), ptr(status), stream_ptr()),
          "sw_ars_rollouts_multi_f64")
    return returns


def _multi_update_shapes(p, returns, deltas, policy, moments, counted, running, mean, inv_std, sigma_out):
    """(S, n_dir, moment rows, on) of a multi-agent update: returns [S, 2N], deltas [S, N, m, d] and _update_state's
    behind (S,); `counted`: the moments hold at least the moments_blocks(2N) rows that N directions fill."""
    on = _gpu(returns, "returns", 2)
    S, n_dir = _tensor(returns, "returns", (_Min(1), _Min(2)), on).shape
    n_dir //= 2
    _tensor(returns, "returns", (S, 2 * n_dir), on)
    _tensor(deltas, "deltas", (S, n_dir, p.m, p.d), on)
    _update_state(p, (S,), on, policy, running, mean, inv_std, sigma_out)
    min_rows = moments_blocks(2 * n_dir) if counted and running is not None else 0
    return S, n_dir, _update_moments(p, (S,), on, moments, running, min_rows), on


def ars_update_multi(p: SwParams, returns, deltas, policy, alpha: float, b: float, top_b: int = 0,
                     moments=None, running=None, n_new_states: int = 0, mean=None, inv_std=None,
                     sigma_out=None):
    """ars_update for S agents in ONE launch (sw_ars_update_multi_f64), in place: returns [S, 2N], deltas
    [S, N, m, d], policy [S, m, d]; with `running` ([S, 1 + 2d]) also moments [S, rows, 2d], mean and inv_std
    [S, d]; sigma_out [S] or None."""
    require_gpu()
    S, n_dir, n_rows, _ = _multi_update_shapes(p, returns, deltas, policy, moments, False, running, mean, inv_std,
                                               sigma_out)
    check(load().sw_ars_update_multi_f64(ctypes.byref(p), S, n_dir, ptr(returns), ptr(deltas), ptr(policy),
                                         float(alpha), float(b), int(top_b), ptr(moments), n_rows, ptr(running),
                                         int(n_new_states), ptr(mean), ptr(inv_std), ptr(sigma_out), stream_ptr()),
          "sw_ars_update_multi_f64")
    return policy


def ars_gate_multi(p_base: SwParams, H: int, policy, deltas, nu: float, sim, sim_thresh, mean=None, inv_std=None,
                   returns=None, status=None, admit=None):
    """ars_gate for S agents in ONE launch (sw_ars_gate_multi_f64), every agent in a simulator and against a threshold
    of its own: policy [S, m, d], deltas [S, N, m, d], sim [S, 3] = each agent's (l_i, m_i, k), sim_thresh [S];
    n, h, the direction and the flags of every simulator come from p_base.  Returns admit (int32 [S, N]); `returns`
    ([S, 2N]) and `status` (int32 [S, 2N]) receive the simulator returns and status codes, row a as ars_gate gives
    them for agent a.  A simulator that breaks the parameter rule: SW_STATUS_PARAM, nothing admitted."""
    require_gpu()
    S, N, on = _multi_shapes(p_base, policy, deltas, mean, inv_std)
    _tensor(sim, "sim", (S, 3), on)
    _tensor(sim_thresh, "sim_thresh", (S,), on)
    returns = _out(returns, "returns", (S, 2 * N), on)
    _opt(status, "status", (S, 2 * N), on, _I32)
    admit = _out(admit, "admit", (S, N), on, _I32)
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
    on = _gpu(admit, "admit", 2)
    S, N = _tensor(admit, "admit", (_Min(1), _Min(1)), on, _I32).shape
    _tensor(deltas, "deltas", (S, N, p.m, p.d), on)
    _opt(status, "status", (S, 2 * N), on, _I32)
    count = _out(count, "count", (S,), on, _I32)
    order = _out(order, "order", (S, N), on, _I32)
    packed = _out(packed, "packed", (S, N, p.m, p.d), on, fill=0.0)
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
    S, N, on = _multi_shapes(p, policy, deltas, mean, inv_std)
    _tensor(count, "count", (S,), on, _I32)
    if moments is not None:
        _tensor(moments, "moments", (S, moments_blocks(2 * N), 2 * p.d), on)
    _opt(status, "status", (S, 2 * N), on, _I32)
    returns = _out(returns, "returns", (S, 2 * N), on, fill=float("nan"))
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
    S, n_dir, n_rows, on = _multi_update_shapes(p, returns, deltas, policy, moments, True, running, mean, inv_std,
                                                sigma_out)
    _tensor(count, "count", (S,), on, _I32)
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
    A, N, on = _multi_shapes(p_real, policy, deltas, None, None)
    _tensor(gated, "gated", (A,), on, _I32)
    _tensor(sim, "sim", (A, 3), on)
    _tensor(sim_thresh, "sim_thresh", (A,), on)
    _tensor(real_thresh, "real_thresh", (A,), on)
    _opt(cost_trace, "cost_trace", (H, A, 2 * N), on)
    _opt(cost_max, "cost_max", (A, 2 * N), on)
    for name, t in (("first_refused", first_refused), ("violations", violations), ("status", status)):
        _opt(t, name, (A, 2 * N), on, _I32)
    returns = _out(returns, "returns", (A, 2 * N), on)
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
    on = _gpu(gamma, "gamma", 1)
    A = _tensor(gamma, "gamma", (_Min(1),), on).shape[0]
    _tensor(alpha, "alpha", (A,), on)
    _tensor(noise, "noise", (A, n_iter, p.m), on)
    _tensor(weights, "weights", (A, p.n, cacla_net_doubles(p.n)), on)
    _tensor(state, "state", (A, p.d), on)
    _opt(actor_updates, "actor_updates", (A,), on, _I32)
    _opt(status, "status", (A,), on, _I32)
    rewards = _out(rewards, "rewards", (A, n_iter), on)
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
    on = _gpu(gathered, "gathered", 1)
    _tensor(gathered, "gathered", (world * (2 * chunk + rows_chunk * 2 * p.d),), on)
    _update_shapes(p, on, n_dir, deltas, policy, running, mean, inv_std, sigma_out)
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
        raise SwimmerHipError("sw_cov_acc_doubles: bad arguments")
    return n


def new_cov_acc(p: SwParams, n_roll: int, H: int, device):
    return torch.zeros(cov_acc_doubles(p, n_roll, H), dtype=torch.float64, device=device)


def traj_moments(p: SwParams, traj, acc=None):
    """acc[:1 + d + d*d] += {count, sum(s-c), sum((s-c)(s-c)^T)} over traj [H, d, n_roll];
    acc = new_cov_acc(p, n_roll, H, device) (sums + scratch), reusable for further passes of
    the same shape.  Deterministic (no floating-point atomics)."""
    require_gpu()
    on = _gpu(traj, "traj", 3)
    H, _, n_roll = _tensor(traj, "traj", (_ANY, p.d, _ANY), on).shape
    acc = _out(acc, "acc", (_Min(cov_acc_doubles(p, n_roll, H)),), on, fill=0.0)
    check(load().sw_traj_moments_f64(ctypes.byref(p), n_roll, H, ptr(traj), ptr(acc),
                                     stream_ptr()), "sw_traj_moments_f64")
    return acc


class ArsPipeline(object):
    """Handle of a native sw_ars_pipeline (include/swimmer_hip.h): the ring-buffered
    copy stream + progress flag + ride-along covariance schedule of one ARS iteration,
    enqueued from C.  rollouts() and update() are the training loop's per-iteration calls and the path bench.py's
    aux_host_cost times: their device tensors are the agent's own buffers, allocated once, and go to the library
    unchecked -- the one exception to this module's argument check."""

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
            raise SwimmerHipError("deltas_host must be a contiguous pinned CPU tensor")
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
    on = _gpu(params, "params", 2)
    A = _tensor(params, "params", (lqr_param_doubles(ns, na), _Min(1)), on).shape[1]
    _tensor(noise, "noise", (n_iter, na, A), on)
    _tensor(F, "F", (na, ns, A), on)
    _tensor(V, "V", (ns, A), on)
    _tensor(state, "state", (ns, A), on)
    _tensor(last, "last", (ns + na + 1, A), on)
    _tensor(counters, "counters", (3, A), on, _I32)
    _tensor(status, "status", (A,), on, _I32)
    _opt(rec_state, "rec_state", (n_iter, ns, A), on)
    _opt(rec_action, "rec_action", (n_iter, na, A), on)
    _opt(rec_reward, "rec_reward", (n_iter, A), on)
    _opt(rec_admitted, "rec_admitted", (n_iter, A), on, torch.uint8)
    check(load().sw_lqr_cacla_run_f64(int(ns), int(na), A, int(n_iter), 1 if safe else 0, int(threshold), int(cost),
                                      ptr(params), ptr(noise), ptr(F), ptr(V), ptr(state), ptr(last), ptr(counters),
                                      ptr(status), ptr(rec_state), ptr(rec_action), ptr(rec_reward),
                                      ptr(rec_admitted), stream_ptr()), "sw_lqr_cacla_run_f64")


def __getattr__(name):
    """kernels.rlglue_ars_run: the checked wrapper of sw_rlglue_ars_run_f64.  It lives next to the classes that use it
    (rlglue/kernels.py, as cacla/safe_kernels.py and ars/ensemble_kernels.py do) and is reachable from here under the
    name its siblings have.  kernels.safe_ars_rollouts_ensemble (safe_ars/ensemble_kernels.py) likewise."""
    if name == "rlglue_ars_run":
        from .rlglue.kernels import rlglue_ars_run
        return rlglue_ars_run
    if name == "safe_ars_rollouts_ensemble":
        from .safe_ars.ensemble_kernels import safe_ars_rollouts_ensemble
        return safe_ars_rollouts_ensemble
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
