"""Generated cases for every compiled instantiation of the single-agent rollout kernels behind sw_rollout_f64 and
sw_ars_rollouts_f64 -- the roots of the suite's tree of bit-equalities: the multi-agent, gate, counted and safe-batch
tests compare with these launches, so a wrong instantiation here is one they would agree with.  Inputs and references
only, no GPU: tests/test_rollout_matrix_cpu.py checks on the oracle alone that the cases exercise what
tests/test_rollout_matrix_gpu.py compares.

INSTANTIATIONS lists the 88 kernels, the twin model's rollout_kernel<N, ARS, true> included, with the launch that
reaches each: entry point, flags, environment, and whether traj / moments are passed (the dispatch rules:
plan_rollouts, launch_oct3, launch_quad3, launch_row, launch_lane).

The reference is oracle.swimmer_oracle on the "realworld" parameters with direction (0.6, -0.8): a swapped Gdot
component shows in every trajectory, and in the returns of the launches with start states (from rest and over these
horizons the returns themselves are ~ 1e-8).  ARS policies are built here in NumPy, P + nu delta_i for rollout 2i and P - nu delta_i
for rollout 2i + 1 with i counted from dir_begin; the deltas array has rows before and behind the slice that a launch
uses, filled with values that would show in every trajectory if read.

THE TWIN MODEL (FLAG_MODEL_TWIN, csrc/swimmer_twin.h: the reference's native RL-Glue swimmer) is the form "twin": it
always runs in the lane form, so its shapes are the lane form's, all of them.  Its reference steps oracle.twin_step
(oracle/twin_oracle.c, pinned entry by entry to the reference's recorded system in tests/test_twin.py) from Python:
per step u = (P diag(inv_std)) (s - mean), the return the sum of the rewards, the start 0.001 in every entry where
there is no state0.  Parameters: the second of step_matrix_cases.TWIN_SETS, (0.8, 1.2, 10.2) with h = 0.003 and the
same direction (0.6, -0.8).  From the 0.001 start the returns are ~ 1e-3, not a rounding residue: a swapped Gdot
component shows in the returns of the ARS launches as well.  The step itself is pinned at every n by
tests/test_step_matrix_gpu.py; what these cases add is everything the lane body wraps around it -- the P +- nu delta
prologue, the whitening fold and its bias, the start, the stores, the moment butterfly (which centres the angle
columns on pi/2 for both models: moment_rows is the same).

SHAPES.  The smallest that still reach each mechanism:
 * horizons HORIZONS at 21 rollouts (ARS: 11 directions = 22): row and quad trips are 4 steps, the mirror-quad trip 8
   with tails of 4, 2 and 1; 21 and 22 are a full workgroup of 16 rollouts and a partial one with a partial wave in
   every form;
 * batch sizes BATCHES at H = 13 (ARS: N_DIRS directions from DIR_BEGINS); the lane form also LANE_BATCHES (ARS:
   LANE_N_DIRS), one rollout per lane of a 64-lane workgroup;
 * plain rollouts from the reset state and from start states (angles in (-pi, pi), |thetadot| <= 2), V1 and V2.

LOOP CROSSINGS (crossing_case, n = 4..8).  The row kernel runs a wave's steps in trips of four without a range check
while 4 h |thetadot| <= 0.04 for all of the wave's rollouts, and step by step with a check inside while not
(too_fast, csrc/swimmer_rollout_row.inc); loops_of() restates that control on the oracle's trajectory.  One case per n,
14 rollouts, all policies P +- nu delta so that the plain and the ARS entry point run the same ones:
   wave 0  rollouts 0..3    from rest; rollout 0's policy (2 P) drives it past 10 rad/s: unchecked -> checked
   wave 1  rollouts 4..7    rollout 5 (policy ~ 0) starts with one segment a little above 10 rad/s and slows down:
                            checked -> unchecked, at a step that need not be a multiple of four; rollout 4 (2 P, from
                            rest) takes the wave back: unchecked -> checked at a trip start that is none either
   wave 2  rollouts 8..11   rollout 8 starts with one segment at CROSS_FAST rad/s; 9, 10, 11 stay below 10 rad/s: the
                            wave is in the checked loop for one rollout's sake
   wave 3  rollouts 12, 13  a partial wave that never leaves the unchecked trips
The ARS entry point has no start state: there every rollout starts from rest, wave 1 only goes unchecked -> checked
and wave 2 becomes mixed once rollout 8 (2 P) has passed 10 rad/s.  CROSSING holds, per n, the seed, gain, start speed
and horizon that a search on the oracle found to meet the conditions of tests/test_rollout_matrix_cpu.py.
"""
import collections
import functools
import zlib

import numpy as np

from conftest import PARAM_SETS
from oracle import swimmer_oracle as oracle
from swimmer_amd import _lib

import step_matrix_cases

L_I, M_I, K, H_STEP = PARAM_SETS["realworld"]
DIRECTION = (0.6, -0.8)
TWIN_PARAMS = step_matrix_cases.TWIN_SETS[1]       # (l_i, m_i, k, h, direction) of the twin cases
TWIN_START = 0.001            # kTwinStart: every entry of the twin's start state (env_start)
TWIN_FLAGS = _lib.FLAG_MODEL_TWIN | _lib.FLAG_ROLLOUT_LANE
TOL = 1e-9                    # relative to max(1, |ref|): the project's bound for runs of up to 1000 steps (TRAJ_TOL)
STABLE = 1e-10                # what inputs scaled by 1 + 1e-13 may move the oracle's own trajectory
MOM_GROUP = 16                # rollouts per V2 moment row (kMomGroup)
TRIP_SLACK = 0.04             # sw::kTripSlack: a trip of four steps may move an angle this far unchecked

# ------------------------------------------------------------------------------------------------ instantiations
Inst = collections.namedtuple("Inst", "symbol form n ars traj mom flags env")
# traj / mom: True / False = the pointer must (not) be passed; None = a run-time argument of the kernel (lane form)


def _instantiations():
    b = lambda x: int(bool(x))
    out = []
    for n in range(4, 9):
        for ars in (0, 1):
            for traj in (0, 1):
                for mom in (0, 1):
                    out.append(Inst(f"rollout_row_kernelILi{n}ELb{ars}ELb{traj}ELb{mom}E", "row", n, b(ars), b(traj),
                                    b(mom), 0, None))
    for ars in (0, 1):
        for traj in (0, 1):
            for mom in (0, 1):
                # capture + moments reach rollout_oct3_kernel only with FLAG_CAPTURE_SPLIT
                flags = _lib.FLAG_CAPTURE_SPLIT if traj and mom else 0
                out.append(Inst(f"rollout_oct3_kernelILb{ars}ELb{traj}ELb{mom}E", "oct3", 3, b(ars), b(traj), b(mom),
                                flags, None))
                # the quad kernel takes small batches only with SWIMMER_N3_KERNEL=quad (read once per process)
                out.append(Inst(f"rollout_quad3_kernelILb{ars}ELb{traj}ELb{mom}E", "quad3", 3, b(ars), b(traj), b(mom),
                                0, "quad"))
        out.append(Inst(f"rollout_octp3_kernelILb{ars}E", "oct3", 3, b(ars), 1, 1, _lib.FLAG_CAPTURE_PACKED_V1, None))
        out.append(Inst(f"rollout_octl3_kernelILb{ars}E", "oct3", 3, b(ars), 1, 1, 0, None))
    for n in range(2, 9):
        for ars in (0, 1):
            out.append(Inst(f"rollout_kernelILi{n}ELb{ars}ELb0E", "lane", n, b(ars), None, None,
                            _lib.FLAG_ROLLOUT_LANE, None))
            out.append(Inst(f"rollout_kernelILi{n}ELb{ars}ELb1E", "twin", n, b(ars), None, None, TWIN_FLAGS, None))
    return tuple(out)


INSTANTIATIONS = _instantiations()
KERNEL_NAMES = ("rollout_row_kernel", "rollout_oct3_kernel", "rollout_octp3_kernel", "rollout_octl3_kernel",
                "rollout_quad3_kernel", "rollout_kernelILi")

# the cases of the GPU test: (form, n).  The n = 3 cases run on the quad kernel in a child process.
FORMS = (("oct3", 3),) + tuple(("row", n) for n in range(4, 9)) + tuple(("lane", n) for n in range(2, 9)) + \
    tuple(("twin", n) for n in range(2, 9))
LANE_FORMS = ("lane", "twin")                      # one rollout per lane of a 64-lane workgroup


def variants(form):
    """The launches of one shape: (name, traj, moments, flags) -- every (TRAJ, MOM) combination the form has."""
    flags = {"lane": _lib.FLAG_ROLLOUT_LANE, "twin": TWIN_FLAGS}.get(form, 0)
    out = [("none", False, False, flags), ("traj", True, False, flags), ("mom", False, True, flags),
           ("traj_mom", True, True, flags)]
    if form == "oct3":          # capture + moments: the lean packed kernel (default), the first packed one, the split one
        out += [("traj_mom_packed_v1", True, True, _lib.FLAG_CAPTURE_PACKED_V1),
                ("traj_mom_split", True, True, _lib.FLAG_CAPTURE_SPLIT)]
    return tuple(out)


def instantiation_of(form, n, ars, traj, mom, flags, quad_env=False):
    """The entry of INSTANTIATIONS that a launch reaches."""
    if form == "oct3" and quad_env:
        form, flags = "quad3", 0
    hits = [i for i in INSTANTIATIONS if i.form == form and i.n == n and i.ars == bool(ars)
            and i.traj in (None, bool(traj)) and i.mom in (None, bool(mom))
            and (i.flags == flags or not (traj and mom and form == "oct3"))]
    assert len(hits) == 1, (form, n, ars, traj, mom, flags, hits)
    return hits[0]


# ------------------------------------------------------------------------------------------------ shapes
HORIZONS = (0, 1, 3, 4, 5, 7, 8, 9, 13, 16, 17)
R_AT_HORIZONS, DIRS_AT_HORIZONS = 21, 11
BATCHES = (1, 3, 4, 5, 15, 16, 17, 33)
H_AT_BATCHES = 13
LANE_BATCHES = (1, 63, 64, 65)
N_DIRS = (1, 2, 7, 8, 9)
DIR_BEGINS = (0, 3)
LANE_N_DIRS = (31, 32, 33)    # 62, 64 and 66 rollouts
NU = 0.05
EXTRA_ROWS = 2                # deltas has n_dir + EXTRA_ROWS rows behind the slice: a kernel that takes a rollout's index
                              # for its direction's still reads what the test allocated, and reads poison
POISON = 1e3                  # scale of the rows of deltas that no launch may read


def plain_shapes(form):
    """(H, R, with_state0) of the sw_rollout_f64 launches of a case."""
    sizes = [(H, R_AT_HORIZONS) for H in HORIZONS] + [(H_AT_BATCHES, R) for R in BATCHES]
    if form in LANE_FORMS:
        sizes += [(H_AT_BATCHES, R) for R in LANE_BATCHES]
    return tuple((H, R, s0) for H, R in sizes for s0 in (True, False))


def ars_shapes(form):
    """(H, n_dir, dir_begin) of the sw_ars_rollouts_f64 launches of a case."""
    out = [(H, DIRS_AT_HORIZONS, DIR_BEGINS[1]) for H in HORIZONS]
    out += [(H_AT_BATCHES, nd, db) for nd in N_DIRS for db in DIR_BEGINS]
    if form in LANE_FORMS:
        out += [(H_AT_BATCHES, nd, DIR_BEGINS[1]) for nd in LANE_N_DIRS]
    return tuple(out)


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def model_of(form):
    return "twin" if form == "twin" else "gym"


def model_params(model="gym"):
    """(l_i, m_i, k, h, direction) of a model's cases."""
    return TWIN_PARAMS if model == "twin" else (L_I, M_I, K, H_STEP, DIRECTION)


def oracle_params(n, model="gym"):
    return oracle.OracleParams.make(n, *model_params(model))


def reset_state(n, model="gym"):
    if model == "twin":
        return np.full(2 * n + 2, TWIN_START)
    s = np.zeros(2 * n + 2)
    s[2::2] = np.pi / 2
    return s


def _whitening(rs, d, v2):
    if not v2:
        return None, None
    mean = 0.05 * rs.standard_normal(d)
    mean[2::2] += np.pi / 2
    return mean, rs.uniform(0.3, 2.0, d)


def start_states(rs, R, n):
    st = np.empty((R, 2 * n + 2))
    st[:, 0:2] = rs.uniform(-0.5, 0.5, (R, 2))
    st[:, 2::2] = rs.uniform(-np.pi, np.pi, (R, n))
    st[:, 3::2] = rs.uniform(-2, 2, (R, n))
    return st


def _model_key(model):
    return () if model == "gym" else (model,)          # the Gym cases keep the streams their records were made with


def plain_inputs(n, H, R, with_state0, v2, model="gym"):
    """dict(n, H, model, policies [R, m, d], state0 [R, d] or None, mean, var [d] or None)."""
    d, m = 2 * n + 2, n - 1
    rs = _rs("plain", n, H, R, with_state0, v2, *_model_key(model))
    policies = 0.3 * rs.uniform(-1, 1, (R, m, d))
    mean, var = _whitening(rs, d, v2)
    return dict(n=n, H=H, model=model, policies=policies, state0=start_states(rs, R, n) if with_state0 else None,
                mean=mean, var=var)


def ars_policies(policy, deltas, nu, dir_begin, n_dir):
    """P + nu delta_i (rollout 2i), P - nu delta_i (rollout 2i + 1), i from dir_begin: [2 n_dir, m, d]."""
    step = nu * deltas[dir_begin:dir_begin + n_dir]
    return np.stack([policy + step, policy - step], axis=1).reshape((2 * n_dir,) + policy.shape)


def ars_inputs(n, H, n_dir, dir_begin, v2, model="gym"):
    """dict(n, H, model, policy [m, d], deltas [dir_begin + 2 n_dir + EXTRA_ROWS, m, d], nu, dir_begin, n_dir, policies,
    state0 = None, mean, var)."""
    d, m = 2 * n + 2, n - 1
    rs = _rs("ars", n, H, n_dir, dir_begin, v2, *_model_key(model))
    policy = 0.2 * rs.uniform(-1, 1, (m, d))
    deltas = POISON * (1 + rs.rand(dir_begin + 2 * n_dir + EXTRA_ROWS, m, d))
    deltas[dir_begin:dir_begin + n_dir] = rs.standard_normal((n_dir, m, d))
    mean, var = _whitening(rs, d, v2)
    return dict(n=n, H=H, model=model, policy=policy, deltas=deltas, nu=NU, dir_begin=dir_begin, n_dir=n_dir,
                policies=ars_policies(policy, deltas, NU, dir_begin, n_dir), state0=None, mean=mean, var=var)


def twin_step(p, state, u):
    """One step of the twin oracle: (next state, reward)."""
    return oracle.twin_step(p, state, u)


def twin_rollout(p, H, policy, mean, var, start):
    """H steps of the twin oracle under a linear policy: u = (P diag(var ** -0.5)) (s - mean), plain P s without
    whitening; (the sum of the rewards, traj [H, d])."""
    W = policy if mean is None else policy * var ** -0.5
    s, total, traj = np.array(start, dtype=np.float64), 0.0, np.empty((H, start.shape[0]))
    for t in range(H):
        s, rew = twin_step(p, s, W @ (s if mean is None else s - mean))
        total += rew
        traj[t] = s
    return total, traj


def reference(inp, scale=1.0):
    """The oracle on a launch's rollouts: dict(returns [R], traj [R, H, d], final [R, d], start [R, d]).  scale: a
    factor on the policies and the start states (the conditioning check of the CPU test)."""
    n, H, model = inp["n"], inp["H"], inp.get("model", "gym")
    p = oracle_params(n, model)
    policies = inp["policies"] * scale
    R = policies.shape[0]
    start = np.tile(reset_state(n, model), (R, 1)) if inp["state0"] is None else inp["state0"] * scale
    rets, traj = np.empty(R), np.empty((R, H, 2 * n + 2))
    for r in range(R):
        if model == "twin":
            rets[r], traj[r] = twin_rollout(p, H, policies[r], inp["mean"], inp["var"], start[r])
        else:
            rets[r], traj[r] = oracle.rollout(p, H, policies[r], inp["mean"], inp["var"],
                                              None if inp["state0"] is None else start[r])
    return dict(returns=rets, traj=traj, final=traj[:, -1] if H else start, start=start)


def moment_rows(traj):
    """The V2 moment rows of a reference trajectory [R, H, d]: row b = the sums over rollouts 16 b .. 16 b + 15 (the
    valid ones) and all steps of obs - c and of its square, c = pi/2 on the angle columns: (rows [B, 2 d], the sums of
    the absolute terms [B, 2 d])."""
    R, H, d = traj.shape
    c = np.zeros(d)
    c[2::2] = np.pi / 2
    x = traj - c
    B = (R + MOM_GROUP - 1) // MOM_GROUP
    rows, scale = np.zeros((B, 2 * d)), np.zeros((B, 2 * d))
    for b in range(B):
        blk = x[MOM_GROUP * b:MOM_GROUP * (b + 1)].reshape(-1, d)
        rows[b] = np.concatenate([blk.sum(0), (blk * blk).sum(0)])
        scale[b] = np.concatenate([np.abs(blk).sum(0), (blk * blk).sum(0)])
    return rows, scale


# ------------------------------------------------------------------------------------------------ loop crossings
UNCHECKED, CHECKED = 0, 1
CROSS_R, CROSS_DIRS, CROSS_NU = 14, 7, 0.5
CROSS_FAST = 25.0             # rad/s of rollout 8's spun segment
# n: (seed, gain of P's angle columns, start speed of rollout 5's segment in rad/s, H)
CROSSING = {
    4: (0, 6.0, 10.15, 48),
    5: (0, 8.0, 10.3, 48),
    6: (0, 8.0, 10.3, 48),
    7: (0, 8.0, 10.15, 48),
    8: (0, 10.0, 10.3, 48),
}


def make_crossing(n, seed, gain, start_speed, H):
    d, m = 2 * n + 2, n - 1
    rs = _rs("crossing", n, seed)
    P = 0.1 * rs.uniform(-1, 1, (m, d))
    for i in range(m):                                    # from rest the torque of joint i is pi/2 times this gain
        P[i, 2 + 2 * i] = gain * rs.uniform(0.6, 1.0) * (1 if i % 2 == 0 else -1)
    deltas = 0.05 * rs.standard_normal((CROSS_DIRS, m, d))
    for i in (0, 2, 4):                                   # rollouts 0, 4, 8: ~ 2 P; rollouts 1, 5, 9: ~ 0
        deltas[i] += P / CROSS_NU
    # (rows behind the slice as in ars_inputs: none is read)
    deltas = np.concatenate([deltas, POISON * (1 + rs.rand(CROSS_DIRS + EXTRA_ROWS, m, d))])
    state0 = np.tile(reset_state(n), (CROSS_R, 1))
    state0[5, 3 + 2 * (n // 2)] = start_speed
    state0[8, 3 + 2 * (n // 2 - 1)] = CROSS_FAST
    return dict(n=n, H=H, policy=P, deltas=deltas, nu=CROSS_NU, dir_begin=0, n_dir=CROSS_DIRS,
                policies=ars_policies(P, deltas, CROSS_NU, 0, CROSS_DIRS), state0=state0, mean=None, var=None)


@functools.lru_cache(maxsize=None)
def crossing_case(n, from_rest=False):
    """The loop-crossing launch of n.  from_rest: as the ARS entry point runs it (no start state)."""
    inp = make_crossing(n, *CROSSING[n])
    if from_rest:
        inp = dict(inp, state0=None)
    return inp


def loops_of(thetadot_before, h=H_STEP):
    """The row kernel's loop control (csrc/swimmer_rollout_row.inc) for one wave.  thetadot_before [H, rollouts of the
    wave, n]: every rollout's angular velocities BEFORE each step.  Returns (loop [H]: UNCHECKED or CHECKED per step,
    margin: the smallest |4 h |thetadot| - 0.04| over the tests that were evaluated)."""
    H = thetadot_before.shape[0]
    travel = (4.0 * h) * np.abs(thetadot_before).reshape(H, -1).max(axis=1)
    loop, margin = np.empty(H, dtype=int), np.inf

    def too_fast(t):
        nonlocal margin
        margin = min(margin, abs(travel[t] - TRIP_SLACK))
        return travel[t] > TRIP_SLACK
    t = 0
    while t < H:
        while t < H:                                      # unchecked trips of (up to) four steps
            if too_fast(t):
                break
            t_end = min(H, t + 4)
            loop[t:t_end] = UNCHECKED
            t = t_end
        while t < H and too_fast(t):                      # checks inside every step
            loop[t] = CHECKED
            t += 1
    return loop, margin


def wave_loops(inp, ref):
    """loops_of for every wave (four rollouts) of a launch: [(loop [H], margin, speed [H, rollouts of the wave]: the
    largest |thetadot| of each rollout before each step)]."""
    H = inp["H"]
    before = np.concatenate([ref["start"][:, None, :], ref["traj"][:, :H - 1, :]], axis=1)[:, :, 3::2]   # [R, H, n]
    out = []
    for w in range(0, before.shape[0], 4):
        thd = before[w:w + 4].transpose(1, 0, 2)
        out.append(loops_of(thd) + (np.abs(thd).max(axis=2),))
    return out
