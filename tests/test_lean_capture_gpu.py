"""n = 3 rollouts with trajectory capture AND V2 moments: the lean mode of the packed record form (rollout_octl3_kernel,
csrc/swimmer_rollout_octp3.inc with SW_OCTP_LEAN 1: the default of such a launch) against the two kernels it stands
beside -- the first packed kernel (rollout_octp3_kernel, FLAG_CAPTURE_PACKED_V1 / rollout_kernel="packed_v1") and the
three-store kernel (rollout_oct3_kernel<.., true, true>, FLAG_CAPTURE_SPLIT / rollout_kernel="split").

The claim is BIT identity of every output -- returns, status, trajectory, final state, moment rows -- so every array is
compared by its bit patterns (test_packed_capture_gpu.same_bits: NaN positions as a mask, the rest as int64).

What is new in the lean mode, and what the cases are for:
* WHERE A STORE GOES.  The scalar offset of a step's store is its position in the trip times the slab (seven pinned
  registers and the constant 0), the trip's base rides in the vector offset and is bumped once per trip -- by 8, 4 or
  2 slabs, by nothing after the single last step.  A wrong bump shows after a trip boundary or in a tail loop:
  H in {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 31, 40} (every combination of the 8 / 4 / 2 / 1 tails, up to five
  main-loop trips) at 24 rollouts.  The trajectory buffer is one step longer than the launch writes and pre-filled
  with a sentinel: every cell of the H steps must have been written, the guard step behind them must not.  The
  launches go through the C ABI directly, because H = 0 needs a non-null trajectory pointer to reach the kernel.
* PARTIAL WAVES AND WORKGROUPS.  n_roll in {1, 7, 8, 9, 16, 17, 130} at H = 19 (8 + 8 + 2 + 1), with a start state and
  a non-trivial mean / inv_std; the ARS form has no start state and launches 2 n_dir rollouts, so there the seven
  sizes are the direction counts (2 .. 260 rollouts: the same situations), from a non-zero dir_begin.
* THE VCC BRANCH TAKEN.  The fast-spinning start states of test_packed_capture_gpu.py (an angle leaves [-pi/4, pi/4]
  every few steps), a rollout that ends in SW_STATUS_RANGE with a NaN return, and a wave in which ONE rollout's
  lanes leave the interval while the others rest inside it (the lane mask in vcc is neither empty nor full).
* THE PIPELINE.  Three ARSAgent(full_covariance=True) iterations, kernels "auto", "packed_v1" and "split"."""
import ctypes

import numpy as np
import pytest
import torch

from test_packed_capture_gpu import D, M, STATUS_RANGE, dev, same_bits

pytestmark = pytest.mark.gpu

ADDRESSING_H = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 31, 40)
PARTIAL_R = (1, 7, 8, 9, 16, 17, 130)
SENTINEL = -7.0


@pytest.fixture(scope="module")
def sw():
    import swimmer_amd
    swimmer_amd._lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return swimmer_amd


def variants(sw):
    return (("lean", 0), ("packed_v1", sw._lib.FLAG_CAPTURE_PACKED_V1), ("split", sw._lib.FLAG_CAPTURE_SPLIT))


def filled(shape, value=SENTINEL, dtype=torch.float64):
    return torch.full(shape, value, dtype=dtype, device="cuda:0")


def read_back(H, ret, status, traj, mom, fin=None):
    torch.cuda.synchronize()
    out = {"returns": ret.cpu().numpy(), "status": status.cpu().numpy(), "traj": traj[:H].cpu().numpy(),
           "guard": traj[H].cpu().numpy(), "moments": mom.cpu().numpy()}
    if fin is not None:
        out["final_state"] = fin.cpu().numpy()
    return out


def plain_outputs(sw, flags, H, pol, state0, mean, inv_std):
    """sw_rollout_f64 with every output, through the C ABI; the trajectory buffer has a guard step behind step H - 1."""
    from swimmer_amd._lib import check, load, ptr, stream_ptr
    R = pol.shape[0]
    p = sw.SwParams.make(3, 0.8, 1.2, 10.2, 1e-3, (0.6, -0.8), flags=flags)
    traj, fin, ret = filled((H + 1, D, R)), filled((D, R)), filled((R,))
    mom = filled((sw.kernels.moments_blocks(R), 2 * D))
    status = filled((R,), -1, torch.int32)
    check(load().sw_rollout_f64(ctypes.byref(p), R, H, ptr(pol), ptr(mean), ptr(inv_std), ptr(state0), ptr(ret),
                                ptr(traj), ptr(fin), ptr(mom), ptr(status), stream_ptr()), "sw_rollout_f64")
    return read_back(H, ret, status, traj, mom, fin)


def ars_outputs(sw, flags, H, policy, deltas, nu, dir_begin, n_dir, mean, inv_std):
    from swimmer_amd._lib import check, load, ptr, stream_ptr
    R = 2 * n_dir
    p = sw.SwParams.make(3, 0.8, 1.2, 10.2, 1e-3, flags=flags)
    traj, ret = filled((H + 1, D, R)), filled((R,))
    mom = filled((sw.kernels.moments_blocks(R), 2 * D))
    status = filled((R,), -1, torch.int32)
    check(load().sw_ars_rollouts_f64(ctypes.byref(p), dir_begin, n_dir, H, ptr(policy), ptr(deltas), nu, ptr(mean),
                                     ptr(inv_std), ptr(ret), ptr(traj), ptr(mom), ptr(status), stream_ptr()),
          "sw_ars_rollouts_f64")
    return read_back(H, ret, status, traj, mom)


def compare(sw, run, label):
    """run(flags) -> outputs; the lean kernel's against both others', bit for bit.  Returns the lean kernel's."""
    got = {name: run(flags) for name, flags in variants(sw)}
    for other in ("packed_v1", "split"):
        for key in got[other]:
            same_bits(got["lean"][key], got[other][key], (label, "lean against", other, key))
    assert not (got["lean"]["traj"] == SENTINEL).any(), (label, "a trajectory cell was not written")
    assert (got["lean"]["guard"] == SENTINEL).all(), (label, "a store went behind the last step")
    return got["lean"]


def start_states(rs, R):
    st0 = np.empty((R, D))
    st0[:, 0:2] = rs.uniform(-0.5, 0.5, (R, 2))
    st0[:, 2::2] = rs.uniform(-np.pi, np.pi, (R, 3))
    st0[:, 3::2] = rs.uniform(-2, 2, (R, 3))
    return st0


@pytest.mark.parametrize("H", ADDRESSING_H)
def test_store_addressing_across_trips_and_tails(sw, H):
    R = 24
    rs = np.random.RandomState(800 + H)
    st0 = dev(start_states(rs, R).T)
    pol = dev(0.3 * (2 * rs.rand(R, M, D) - 1))
    mean, inv_std = dev(rs.uniform(-0.2, 0.2, D)), dev(rs.uniform(0.5, 2.0, D))
    out = compare(sw, lambda f: plain_outputs(sw, f, H, pol, st0, mean, inv_std), ("addressing", "H", H))
    assert int(np.abs(out["status"]).sum()) == 0
    # every step's slab holds that step: theta advances by h * thetadot of the step before (checked loosely: the point
    # is WHICH slab a record landed in, the bits are compared above)
    if H >= 2:
        th, thd = out["traj"][:, 2::2, :], out["traj"][:, 3::2, :]
        assert np.abs(th[1:] - (th[:-1] + 1e-3 * thd[:-1])).max() < 1e-9
    n_dir = R // 2
    deltas, policy = dev(rs.randn(2 + n_dir, M, D)), dev(0.2 * (2 * rs.rand(M, D) - 1))
    out = compare(sw, lambda f: ars_outputs(sw, f, H, policy, deltas, 0.05, 2, n_dir, mean, inv_std),
                  ("addressing, ars", "H", H))
    assert int(np.abs(out["status"]).sum()) == 0


@pytest.mark.parametrize("R", PARTIAL_R)
def test_partial_waves_and_workgroups(sw, R):
    H = 19
    rs = np.random.RandomState(900 + R)
    st0 = dev(start_states(rs, R).T)
    pol = dev(0.3 * (2 * rs.rand(R, M, D) - 1))
    mean, inv_std = dev(rs.uniform(-0.2, 0.2, D)), dev(rs.uniform(0.5, 2.0, D))
    out = compare(sw, lambda f: plain_outputs(sw, f, H, pol, st0, mean, inv_std), ("partial", "R", R))
    assert int(np.abs(out["status"]).sum()) == 0
    compare(sw, lambda f: plain_outputs(sw, f, H, pol, None, None, None), ("partial, reset state", "R", R))
    n_dir, dir_begin = R, 3
    deltas, policy = dev(rs.randn(dir_begin + n_dir, M, D)), dev(0.2 * (2 * rs.rand(M, D) - 1))
    for v2 in (True, False):
        out = compare(sw, lambda f: ars_outputs(sw, f, H, policy, deltas, 0.05, dir_begin, n_dir,
                                                mean if v2 else None, inv_std if v2 else None),
                      ("partial, ars", "n_dir", n_dir, "v2", v2))
        assert int(np.abs(out["status"]).sum()) == 0


@pytest.mark.parametrize("R", (7, 17, 33))
def test_fast_spinning_start_takes_the_vcc_branch(sw, R):
    """The inputs of test_packed_capture_gpu.test_fast_spinning_start_takes_the_renormalisation_block: up to 400 rad/s =
    0.4 rad per step, angles up to 50 rad, half of the batch twenty times slower."""
    rs = np.random.RandomState(7 + 3)
    crossings = 0
    for H in (1, 2, 3, 7, 8, 9, 17):
        st0 = np.empty((R, D))
        st0[:, 0:2] = rs.uniform(-0.5, 0.5, (R, 2))
        st0[:, 2::2] = rs.uniform(-50.0, 50.0, (R, 3))
        st0[:, 3::2] = rs.uniform(-400.0, 400.0, (R, 3))
        st0[: R // 2, 3::2] *= 0.05
        pol = dev(0.05 * (2 * rs.rand(R, M, D) - 1))
        start = dev(st0.T)
        out = compare(sw, lambda f: plain_outputs(sw, f, H, pol, start, None, None), ("fast spinning", "R", R, "H", H))
        assert int(np.abs(out["status"]).sum()) == 0
        quadrant = lambda th: np.floor((th + np.pi / 4) / (np.pi / 2))
        crossings += int((quadrant(out["traj"][:, 2::2, :]) != quadrant(st0[:, 2::2].T)[None]).any(axis=0).sum())
    assert crossings > 0, "no angle left its quadrant: the in-loop re-normalisation was never taken"


def test_a_rollout_that_leaves_the_angle_range(sw):
    R = 17
    rs = np.random.RandomState(317)
    for H in (1, 9, 17):
        st0 = np.zeros((R, D))
        st0[:, 2::2] = rs.uniform(-np.pi, np.pi, (R, 3))
        st0[:, 3::2] = rs.uniform(-2, 2, (R, 3))
        bad = R - 1
        st0[bad, 4] = 3.1e9                     # segment 1 of the last rollout: beyond the in-kernel sin / cos range
        pol, start = dev(0.3 * (2 * rs.rand(R, M, D) - 1)), dev(st0.T)
        out = compare(sw, lambda f: plain_outputs(sw, f, H, pol, start, None, None), ("range", "H", H))
        assert out["status"][bad] & STATUS_RANGE and np.isnan(out["returns"][bad])
        assert not (np.delete(out["status"], bad) & STATUS_RANGE).any()
        assert not np.isnan(np.delete(out["returns"], bad)).any()


def test_a_wave_in_which_only_some_lanes_leave_the_interval(sw):
    """Sixteen rollouts = two waves, zero policies, every swimmer at rest with all angles 0 (the middle of the reduced
    interval): nothing moves, no lane ever leaves [-pi/4, pi/4] -- except rollout 3, whose first segment starts at
    300 rad/s (0.3 rad per step: out of the interval within three steps, again and again).  In the steps it leaves,
    the mask in vcc has the bits of some lanes of wave 0 and of no other."""
    R, H, spun = 16, 23, 3
    st0 = np.zeros((R, D))
    st0[spun, 3] = 300.0
    pol, start = dev(np.zeros((R, M, D))), dev(st0.T)
    out = compare(sw, lambda f: plain_outputs(sw, f, H, pol, start, None, None), "mixed wave")
    assert int(np.abs(out["status"]).sum()) == 0
    th = out["traj"][:, 2::2, :]                                  # [H, segment, rollout]
    assert np.abs(th[:, 0, spun]).max() > np.pi / 4, "the spun segment never left the interval"
    rest = np.delete(th, spun, axis=2)
    assert np.abs(rest).max() < np.pi / 4, "a rollout at rest left the interval: the wave was not mixed as intended"


def test_pipeline_auto_against_packed_v1_and_split(sw):
    """Three iterations of the native ARS pipeline with the full covariance riding along in the next rollout launch."""
    ep = sw.EnvParam("LeonSwimmer-Lean", n=3, H=24, l_i=1.0, m_i=1.0, h=1e-3, k=10.0, epsilon=0)
    ap = sw.ARSParam("Lean", V1=False, n_iter=3, H=24, N=8, b=8, alpha=0.0075, nu=0.01, safe=False, threshold=0,
                     initial_w="Zero")
    out = {}
    for kernel in ("auto", "packed_v1", "split"):
        agent = sw.ARSAgent(ep, ap, seed=13, full_covariance=True, rollout_kernel=kernel)
        rets = [np.array(agent.runOneIteration()) for _ in range(3)]
        out[kernel] = {"returns": np.stack(rets), "policy": np.array(agent.policy), "mean": np.array(agent.mean),
                       "std (as 1 / std)": agent._inv_std.cpu().numpy(), "covariance": np.array(agent.covariance)}
    assert np.abs(out["auto"]["policy"]).max() > 0
    for other in ("packed_v1", "split"):
        for key in out[other]:
            same_bits(out["auto"][key], out[other][key], ("pipeline", "auto against", other, key))
