"""n = 3 rollouts with trajectory capture AND V2 moments: the lean kernel with the NEIGHBOUR'S MATRIX ENTRY
(rollout_octs3_kernel, csrc/swimmer_rollout_octp3.inc with SW_OCTP_NEXT_E 1: the default of such a launch) against the
three kernels it stands beside -- the lean kernel before it (rollout_octl3_kernel, FLAG_CAPTURE_LEAN_V1 /
rollout_kernel="lean_v1"), the first packed kernel ("packed_v1") and the three-store kernel ("split").

What is new: a lane takes Q(i+1, i+2) of its rotated 3x3 system from lane i+1 (whose Q(i, i+1) it is) through two DPP
moves instead of forming it from cos(th_i1 - th_i2) and t12.  The claim is BIT identity of every output -- returns,
status, trajectory, final state, moment rows -- so every array is compared by its bit patterns
(test_packed_capture_gpu.same_bits: NaN positions as a mask, the rest as int64); against the lean kernel, which differs
in nothing but that entry, NaNs are compared by their bits as well (no operand is commuted, so the payloads and signs
agree too).  The trajectory buffer is one step longer than a launch writes and pre-filled with a sentinel, as in
test_lean_capture_gpu.py: every cell of the H steps written, the guard step behind them not.

Shapes, the smallest that reach every path:
* H in {0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 33}: the boundaries of the trip of eight (and of a trip of sixteen) with every
  tail; n_roll in {1, 2, 7, 8, 9, 16, 17}: a partial wave, surplus rollouts recomputing the last one, a second
  workgroup.  ARS launches (2 n_dir rollouts, dir_begin 0 and 3) take the sizes as direction counts.
* Start states: from rest, random, one rollout spinning fast enough to cross several quarter turns (the out-of-line
  re-normalisation block), one with a NaN component, one that ends in SW_STATUS_RANGE with a NaN return.
* Three ARSAgent(full_covariance=True) iterations, "auto" against "lean_v1": the riding covariance pass and the update
  see the same data."""
import numpy as np
import pytest
import torch

from test_lean_capture_gpu import SENTINEL, ars_outputs, plain_outputs, start_states
from test_packed_capture_gpu import D, M, STATUS_RANGE, dev, same_bits

pytestmark = pytest.mark.gpu

HORIZONS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 33)
ROLLOUTS = (1, 2, 7, 8, 9, 16, 17)
DIR_BEGINS = (0, 3)


@pytest.fixture(scope="module")
def sw():
    import swimmer_amd
    swimmer_amd._lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return swimmer_amd


def variants(sw):
    return (("auto", 0), ("lean_v1", sw._lib.FLAG_CAPTURE_LEAN_V1), ("packed_v1", sw._lib.FLAG_CAPTURE_PACKED_V1),
            ("split", sw._lib.FLAG_CAPTURE_SPLIT))


def exact_bits(a, b, what):
    """Every bit, those of a NaN included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32),
                          b.view(np.int64 if b.dtype.itemsize == 8 else np.int32)), what


def compare_all(sw, run, label):
    """run(flags) -> outputs; the default kernel's against the three others'.  Returns every kernel's, by name."""
    got = {name: run(flags) for name, flags in variants(sw)}
    for other in ("lean_v1", "packed_v1", "split"):
        for key in got[other]:
            same_bits(got["auto"][key], got[other][key], (label, "auto against", other, key))
    for key in got["lean_v1"]:
        exact_bits(got["auto"][key], got["lean_v1"][key], (label, "auto against lean_v1, NaN bits included", key))
    assert not (got["auto"]["traj"] == SENTINEL).any(), (label, "a trajectory cell was not written")
    assert (got["auto"]["guard"] == SENTINEL).all(), (label, "a store went behind the last step")
    return got


def compare(sw, run, label):
    """compare_all; returns the default kernel's outputs."""
    return compare_all(sw, run, label)["auto"]


@pytest.mark.parametrize("H", HORIZONS)
def test_every_horizon_and_batch_size(sw, H):
    for R in ROLLOUTS:
        rs = np.random.RandomState(1000 * H + R)
        pol = dev(0.3 * (2 * rs.rand(R, M, D) - 1))
        st0 = dev(start_states(rs, R).T)
        mean, inv_std = dev(rs.uniform(-0.2, 0.2, D)), dev(rs.uniform(0.5, 2.0, D))
        out = compare(sw, lambda f: plain_outputs(sw, f, H, pol, None, None, None), ("from rest", "H", H, "R", R))
        assert int(np.abs(out["status"]).sum()) == 0
        out = compare(sw, lambda f: plain_outputs(sw, f, H, pol, st0, mean, inv_std), ("random", "H", H, "R", R))
        assert int(np.abs(out["status"]).sum()) == 0
        n_dir = R
        policy = dev(0.2 * (2 * rs.rand(M, D) - 1))
        for dir_begin in DIR_BEGINS:
            deltas = dev(rs.randn(dir_begin + n_dir, M, D))
            out = compare(sw, lambda f: ars_outputs(sw, f, H, policy, deltas, 0.05, dir_begin, n_dir, mean, inv_std),
                          ("ars", "H", H, "n_dir", n_dir, "dir_begin", dir_begin))
            assert int(np.abs(out["status"]).sum()) == 0


@pytest.mark.parametrize("R", ROLLOUTS)
def test_a_fast_spinning_rollout_crosses_quarter_turns(sw, R):
    """One rollout (the last: in a partial wave its lanes' state is what the surplus lanes recompute) starts with up to
    400 rad/s = 0.4 rad per step on every segment: an angle leaves [-pi/4, pi/4] every few steps."""
    rs = np.random.RandomState(40 + R)
    crossings = 0
    for H in (3, 9, 17, 33):
        st0 = start_states(rs, R)
        st0[R - 1, 2::2] = rs.uniform(-50.0, 50.0, 3)
        st0[R - 1, 3::2] = rs.uniform(200.0, 400.0, 3) * rs.choice([-1.0, 1.0], 3)
        pol, start = dev(0.05 * (2 * rs.rand(R, M, D) - 1)), dev(st0.T)
        out = compare(sw, lambda f: plain_outputs(sw, f, H, pol, start, None, None), ("spinning", "R", R, "H", H))
        assert int(np.abs(out["status"]).sum()) == 0
        quadrant = lambda th: np.floor((th + np.pi / 4) / (np.pi / 2))
        th = out["traj"][:, 2::2, R - 1]                              # [H, segment]
        crossings += len(np.unique(quadrant(th))) - 1
    assert crossings >= 3, "the spun rollout did not cross several quarter turns"


@pytest.mark.parametrize("R", (2, 9, 17))
def test_a_nan_start_component(sw, R):
    """thetadot of segment 1 of one rollout is NaN: its lanes carry NaN through the exchanged entry from step one."""
    rs = np.random.RandomState(60 + R)
    for H in (1, 8, 17):
        st0 = start_states(rs, R)
        bad = R // 2
        st0[bad, 5] = np.nan
        pol, start = dev(0.3 * (2 * rs.rand(R, M, D) - 1)), dev(st0.T)
        out = compare(sw, lambda f: plain_outputs(sw, f, H, pol, start, None, None), ("nan start", "R", R, "H", H))
        assert np.isnan(out["returns"][bad]) and np.isnan(out["traj"][:, :, bad]).any()
        assert not np.isnan(np.delete(out["returns"], bad)).any()
        assert int(np.abs(np.delete(out["status"], bad)).sum()) == 0


@pytest.mark.parametrize("R", (1, 9, 17))
def test_a_rollout_that_ends_in_status_range(sw, R):
    rs = np.random.RandomState(80 + R)
    for H in (1, 9, 16):
        st0 = np.zeros((R, D))
        st0[:, 2::2] = rs.uniform(-np.pi, np.pi, (R, 3))
        st0[:, 3::2] = rs.uniform(-2, 2, (R, 3))
        bad = R - 1
        st0[bad, 4] = 3.1e9                     # segment 1: beyond the in-kernel sin / cos range
        pol, start = dev(0.3 * (2 * rs.rand(R, M, D) - 1)), dev(st0.T)
        got = compare_all(sw, lambda f: plain_outputs(sw, f, H, pol, start, None, None), ("range", "R", R, "H", H))
        out = got["auto"]
        assert out["status"][bad] & STATUS_RANGE and np.isnan(out["returns"][bad])
        for other in ("lean_v1", "packed_v1", "split"):          # the NaN return and the status: the same bits
            exact_bits(out["returns"], got[other]["returns"], ("range", "returns", other))
            exact_bits(out["status"], got[other]["status"], ("range", "status", other))
        assert not (np.delete(out["status"], bad) & STATUS_RANGE).any()
        assert not np.isnan(np.delete(out["returns"], bad)).any()


def test_pipeline_auto_against_lean_v1(sw):
    """Three iterations of the native ARS pipeline with the full covariance riding along in the next rollout launch."""
    ep = sw.EnvParam("LeonSwimmer-NextE", n=3, H=17, l_i=1.0, m_i=1.0, h=1e-3, k=10.0, epsilon=0)
    ap = sw.ARSParam("NextE", V1=False, n_iter=3, H=17, N=8, b=8, alpha=0.0075, nu=0.01, safe=False, threshold=0,
                     initial_w="Zero")
    out = {}
    for kernel in ("auto", "lean_v1"):
        agent = sw.ARSAgent(ep, ap, seed=13, full_covariance=True, rollout_kernel=kernel)
        rets = [np.array(agent.runOneIteration()) for _ in range(3)]
        out[kernel] = {"returns": np.stack(rets), "policy": np.array(agent.policy), "mean": np.array(agent.mean),
                       "std (as 1 / std)": agent._inv_std.cpu().numpy(), "covariance": np.array(agent.covariance)}
    assert np.abs(out["auto"]["policy"]).max() > 0
    for key in out["lean_v1"]:
        assert out["auto"][key].tobytes() == out["lean_v1"][key].tobytes(), ("pipeline", "auto against lean_v1", key)
