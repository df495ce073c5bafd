"""n = 3 rollouts with trajectory capture AND V2 moments: the packed record form (rollout_octp3_kernel: one wave-wide
trajectory store and one moment pair per step, csrc/swimmer_rollout_octp3.inc) against the three-store kernel it
replaces on that path (rollout_oct3_kernel<.., true, true>, kept behind FLAG_CAPTURE_SPLIT / rollout_kernel="split").

The claim is BIT identity of every output -- returns, status, trajectory, final state, moment rows -- so every array is
compared by its bit patterns (NaN positions as a mask, everything else as int64, which also tells -0.0 from 0.0).

Shapes: n_roll in {1, 7, 16, 17, 33} (surplus rollouts inside a wave, a partial second wave, more than one workgroup)
x H in {1, 2, 3, 7, 8, 9, 17} (every remainder of the 8 / 4 / 2 / 1 trip ladder).  The ARS form launches 2 n_dir
rollouts, always an even number: there the five sizes are the DIRECTION counts (2, 14, 32, 34, 66 rollouts: the same
three situations), from a non-zero dir_begin."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ROLL = (1, 7, 16, 17, 33)
HORIZONS = (1, 2, 3, 7, 8, 9, 17)
D, M = 8, 2
STATUS_RANGE = 4


@pytest.fixture(scope="module")
def sw():
    import swimmer_amd
    swimmer_amd._lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return swimmer_amd


def dev(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device="cuda:0")


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype.kind != "f":
        assert np.array_equal(a, b), what
        return
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (what, "NaN positions")
    assert np.array_equal(np.where(na, 0.0, a).view(np.int64), np.where(nb, 0.0, b).view(np.int64)), what


def plain_outputs(sw, flags, H, pol, state0, mean, inv_std):
    """sw_rollout_f64 with every output; buffers pre-filled so that a cell nobody wrote shows."""
    R = pol.shape[0]
    p = sw.SwParams.make(3, 0.8, 1.2, 10.2, 1e-3, (0.6, -0.8), flags=flags)
    traj = torch.full((H, D, R), -7.0, dtype=torch.float64, device="cuda:0")
    fin = torch.full((D, R), -7.0, dtype=torch.float64, device="cuda:0")
    mom = torch.full((sw.kernels.moments_blocks(R), 2 * D), -7.0, dtype=torch.float64, device="cuda:0")
    status = torch.full((R,), -1, dtype=torch.int32, device="cuda:0")
    ret = sw.kernels.rollout(p, H, pol, mean=mean, inv_std=inv_std, state0=state0, traj=traj, final_state=fin,
                             moments=mom, status=status)
    torch.cuda.synchronize()
    return {"returns": ret.cpu().numpy(), "status": status.cpu().numpy(), "traj": traj.cpu().numpy(),
            "final_state": fin.cpu().numpy(), "moments": mom.cpu().numpy()}


def compare_plain(sw, H, pol, state0, mean=None, inv_std=None, label=""):
    packed = plain_outputs(sw, 0, H, pol, state0, mean, inv_std)
    split = plain_outputs(sw, sw._lib.FLAG_CAPTURE_SPLIT, H, pol, state0, mean, inv_std)
    for key in split:
        same_bits(packed[key], split[key], (label, "R", pol.shape[0], "H", H, key))
    assert not (packed["traj"] == -7.0).any(), (label, "a trajectory cell was not written")
    return packed


@pytest.mark.parametrize("R", N_ROLL)
def test_nonzero_start_state(sw, R):
    rs = np.random.RandomState(100 + R)
    for H in HORIZONS:
        st0 = np.empty((R, D))
        st0[:, 0:2] = rs.uniform(-0.5, 0.5, (R, 2))
        st0[:, 2::2] = rs.uniform(-np.pi, np.pi, (R, 3))
        st0[:, 3::2] = rs.uniform(-2, 2, (R, 3))
        pol = dev(0.3 * (2 * rs.rand(R, M, D) - 1))
        mean = dev(rs.uniform(-0.2, 0.2, D))
        inv_std = dev(rs.uniform(0.5, 2.0, D))
        out = compare_plain(sw, H, pol, dev(st0.T), mean, inv_std, "state0 + normalisation")
        assert int(np.abs(out["status"]).sum()) == 0
        compare_plain(sw, H, pol, dev(st0.T), label="state0")
        compare_plain(sw, H, pol, None, label="reset state")


@pytest.mark.parametrize("R", N_ROLL)
def test_fast_spinning_start_takes_the_renormalisation_block(sw, R):
    """The start states of test_fast_spinning_segments_stay_exact (test_hip_parity.py): up to 400 rad/s = 0.4 rad per
    step, angles up to 50 rad, half of the batch twenty times slower -- an angle leaves [-pi/4, pi/4] every few steps."""
    rs = np.random.RandomState(7 + 3)
    crossings = 0
    for H in HORIZONS:
        st0 = np.empty((R, D))
        st0[:, 0:2] = rs.uniform(-0.5, 0.5, (R, 2))
        st0[:, 2::2] = rs.uniform(-50.0, 50.0, (R, 3))
        st0[:, 3::2] = rs.uniform(-400.0, 400.0, (R, 3))
        st0[: R // 2, 3::2] *= 0.05
        pol = dev(0.05 * (2 * rs.rand(R, M, D) - 1))
        out = compare_plain(sw, H, pol, dev(st0.T), label="fast spinning")
        assert int(np.abs(out["status"]).sum()) == 0
        quadrant = lambda th: np.floor((th + np.pi / 4) / (np.pi / 2))
        crossings += int((quadrant(out["traj"][:, 2::2, :]) != quadrant(st0[:, 2::2].T)[None]).any(axis=0).sum())
    assert crossings > 0, "no angle left its quadrant: the in-loop re-normalisation was never taken"


@pytest.mark.parametrize("R", N_ROLL)
def test_a_rollout_that_leaves_the_angle_range(sw, R):
    rs = np.random.RandomState(300 + R)
    for H in HORIZONS:
        st0 = np.zeros((R, D))
        st0[:, 2::2] = rs.uniform(-np.pi, np.pi, (R, 3))
        st0[:, 3::2] = rs.uniform(-2, 2, (R, 3))
        bad = R - 1
        st0[bad, 4] = 3.1e9                     # segment 1 of the last rollout: beyond the in-kernel sin / cos range
        pol = dev(0.3 * (2 * rs.rand(R, M, D) - 1))
        out = compare_plain(sw, H, pol, dev(st0.T), label="range")
        assert out["status"][bad] & STATUS_RANGE and np.isnan(out["returns"][bad])
        assert not (np.delete(out["status"], bad) & STATUS_RANGE).any()
        assert not np.isnan(np.delete(out["returns"], bad)).any()


@pytest.mark.parametrize("n_dir", N_ROLL)
def test_ars_form(sw, n_dir):
    rs = np.random.RandomState(500 + n_dir)
    dir_begin = 3
    deltas = dev(rs.randn(dir_begin + n_dir, M, D))
    policy = dev(0.2 * (2 * rs.rand(M, D) - 1))
    mean = dev(rs.uniform(-0.2, 0.2, D))
    inv_std = dev(rs.uniform(0.5, 2.0, D))
    R = 2 * n_dir
    for H in HORIZONS:
        for v2 in (True, False):
            got = {}
            for name, flags in (("packed", 0), ("split", sw._lib.FLAG_CAPTURE_SPLIT)):
                p = sw.SwParams.make(3, 0.8, 1.2, 10.2, 1e-3, flags=flags)
                traj = torch.full((H, D, R), -7.0, dtype=torch.float64, device="cuda:0")
                mom = torch.full((sw.kernels.moments_blocks(R), 2 * D), -7.0, dtype=torch.float64, device="cuda:0")
                status = torch.full((R,), -1, dtype=torch.int32, device="cuda:0")
                ret = sw.kernels.ars_rollouts(p, H, policy, deltas, 0.05, dir_begin, n_dir,
                                              mean=mean if v2 else None, inv_std=inv_std if v2 else None, traj=traj,
                                              moments=mom, status=status)
                torch.cuda.synchronize()
                got[name] = {"returns": ret.cpu().numpy(), "status": status.cpu().numpy(),
                             "traj": traj.cpu().numpy(), "moments": mom.cpu().numpy()}
            for key in got["split"]:
                same_bits(got["packed"][key], got["split"][key], ("ars", "n_dir", n_dir, "H", H, "v2", v2, key))
            assert not (got["packed"]["traj"] == -7.0).any()
            assert int(np.abs(got["packed"]["status"]).sum()) == 0


def test_pipeline_auto_against_split(sw):
    """Three iterations of the native ARS pipeline with the full covariance riding along in the next rollout launch."""
    ep = sw.EnvParam("LeonSwimmer-Packed", n=3, H=50, l_i=1.0, m_i=1.0, h=1e-3, k=10.0, epsilon=0)
    ap = sw.ARSParam("Packed", V1=False, n_iter=3, H=50, N=8, b=8, alpha=0.0075, nu=0.01, safe=False, threshold=0,
                     initial_w="Zero")
    out = {}
    for kernel in ("auto", "split"):
        agent = sw.ARSAgent(ep, ap, seed=13, full_covariance=True, rollout_kernel=kernel)
        rets = [np.array(agent.runOneIteration()) for _ in range(3)]
        out[kernel] = {"returns": np.stack(rets), "policy": np.array(agent.policy), "mean": np.array(agent.mean),
                       "std (as 1 / std)": agent._inv_std.cpu().numpy(), "covariance": np.array(agent.covariance)}
    assert np.abs(out["auto"]["policy"]).max() > 0
    for key in out["split"]:
        same_bits(out["auto"][key], out["split"][key], ("pipeline", key))
