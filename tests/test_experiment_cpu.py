"""The host side of Experiment / ARSAgentBatch that needs no GPU: the per-seed random streams, the slot layout of a
multi-agent launch, the reference's file names, and the argument errors raised before any device work."""
import ctypes

import numpy as np
import pytest

import swimmer_amd as sw
from swimmer_amd.ars import agent_batch, experiment


def test_seed_streams_draw_what_each_seeded_agent_draws_and_leave_numpy_alone():
    N, m, d = 5, 2, 8
    expected = {}
    for s in (0, 3):
        np.random.seed(s)
        expected[s] = [2 * np.random.rand(N, m, d) - 1 for _ in range(3)]
    np.random.seed(12345)
    before = np.random.get_state()
    streams = agent_batch.SeedStreams([0, 3])
    out = np.empty((2, N, m, d))
    for draw in range(3):
        streams.fill(out)
        assert np.array_equal(out[0], expected[0][draw]), draw
        assert np.array_equal(out[1], expected[3][draw]), draw
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    with pytest.raises(sw.SwimmerHipError):
        streams.fill(np.empty((3, N, m, d)))             # one row per seed
    with pytest.raises(sw.SwimmerHipError):
        streams.fill(np.empty((2, N, m, d), dtype=np.float32))


@pytest.mark.parametrize("n_roll,per_agent", [(2, 16), (14, 16), (16, 16), (18, 32)])
def test_slot_layout_gives_every_agent_whole_moment_rows(n_roll, per_agent):
    S = 3
    agent, local, valid = agent_batch.slot_layout(S, n_roll)
    assert len(agent) == len(local) == len(valid) == S * per_agent
    for slot in range(S * per_agent):
        a, raw = divmod(slot, per_agent)
        assert agent[slot] == a
        assert valid[slot] == (raw < n_roll)
        assert local[slot] == (raw if raw < n_roll else n_roll - 1)   # idle slots recompute the agent's last rollout
    # a 16-slot moment row never holds two agents, and an agent's row i covers its rollouts 16 i .. 16 i + 15
    for row in range(S * per_agent // 16):
        sl = slice(16 * row, 16 * row + 16)
        assert len(set(agent[sl])) == 1
        mine = local[sl][valid[sl]]
        first = 16 * (row % (per_agent // 16))
        assert np.array_equal(mine, np.arange(first, min(first + 16, n_roll)))
    # dense outputs: every (agent, rollout) has exactly one valid slot
    pairs = sorted(zip(agent[valid].tolist(), local[valid].tolist()))
    assert pairs == [(a, r) for a in range(S) for r in range(n_roll)]
    # the lane form pads to its 64-lane workgroups
    agent64, _, valid64 = agent_batch.slot_layout(S, n_roll, agent_batch.SLOT_GRANULE_LANE)
    assert len(agent64) == S * 64 and valid64.sum() == S * n_roll
    with pytest.raises(ValueError):
        agent_batch.slot_layout(0, n_roll)


def test_file_names_follow_the_reference_scheme():
    ep = sw.EnvParam("LeonSwimmer", n=3, H=1000, l_i=1., m_i=1., h=1e-3, k=10., epsilon=0)
    ap = sw.ARSParam("ARS", V1=True, n_iter=300, H=1000, N=1, b=1, alpha=0.01, nu=0.01, safe=False, threshold=0,
                     initial_w="Zero")
    assert experiment.describe(ep, ap) == (
        "LeonSwimmer, n_segments=3, m_i=1.0, l_i=1.0, epsilon=0, deltaT=0.001",
        "ARS, ARS_V1, n_directions=1, deltas_used=1, step_size=0.01, delta_std=0.01")
    assert experiment.file_stem(ep, ap) == (
        "LeonSwimmer-n_segments=3-m_i=1.0-l_i=1.0-epsilon=0-deltaT=0.001-"
        "ARS-ARS_V1-n_directions=1-deltas_used=1-step_size=0.01-delta_std=0.01")
    ep = sw.EnvParam("LeonSwimmer-RealWorld", n=3, H=1000, l_i=.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0.123456)
    ap = sw.ARSParam("RLControl", V1=False, n_iter=100, H=1000, N=8, b=4, alpha=0.0075, nu=0.01, safe=False,
                     threshold=0, initial_w="Zero")
    assert experiment.file_stem(ep, ap) == (
        "LeonSwimmer-RealWorld-n_segments=3-m_i=1.2-l_i=0.8-epsilon=0.1235-deltaT=0.001-"
        "RLControl-ARS_V2-t-n_directions=8-deltas_used=4-step_size=0.0075-delta_std=0.01")


def test_which_path_an_experiment_takes():
    ep = sw.EnvParam("E", n=3, H=10, l_i=1., m_i=1., h=1e-3, k=10., epsilon=0)
    unsafe = sw.ARSParam("A", V1=True, n_iter=1, H=10, N=1, b=1, alpha=0.01, nu=0.01, safe=False, threshold=0,
                         initial_w="Zero")
    safe = sw.ARSParam("A", V1=True, n_iter=1, H=10, N=1, b=1, alpha=0.01, nu=0.01, safe=True, threshold=0,
                       initial_w="Zero")
    assert sw.Experiment(ep).batched(unsafe)
    assert not sw.Experiment(ep).batched(safe)
    assert not sw.Experiment(ep, save_data_path="somewhere/db").batched(unsafe)
    exp = sw.Experiment(ep, "out/", "d", "sd", "sp", "g", 0.1, "t")      # the reference's positional order
    assert (exp.results_path, exp.data_path, exp.save_data_path, exp.save_policy_path, exp.guess_param,
            exp.approx_error, exp.sim_thresh) == ("out/", "d", "sd", "sp", "g", 0.1, "t")
    with pytest.raises(ValueError):
        sw.Experiment(ep).train(0, unsafe)


def test_batch_refuses_what_it_does_not_support_before_touching_the_gpu(tmp_path):
    ep = sw.EnvParam("E", n=3, H=10, l_i=1., m_i=1., h=1e-3, k=10., epsilon=0)
    kw = dict(V1=True, n_iter=1, H=10, N=1, b=1, alpha=0.01, nu=0.01, threshold=0)
    unsafe = sw.ARSParam("A", safe=False, initial_w="Zero", **kw)
    with pytest.raises(NotImplementedError, match="safe=True"):
        sw.ARSAgentBatch(ep, sw.ARSParam("A", safe=True, initial_w="Zero", **kw), [0, 1])
    with pytest.raises(NotImplementedError, match="trajectories"):
        sw.ARSAgentBatch(ep, unsafe, [0, 1], record_trajectories=True)
    with pytest.raises(ValueError, match="at least one seed"):
        sw.ARSAgentBatch(ep, unsafe, [])
    with pytest.raises(sw.SwimmerHipError, match="rollout kernel"):
        sw.ARSAgentBatch(ep, unsafe, [0], rollout_kernel="fastest")
    np.save(tmp_path / "w.npy", np.zeros((3, 3)))
    with pytest.raises(ValueError, match="initial_w"):
        sw.ARSAgentBatch(ep, sw.ARSParam("A", safe=False, initial_w=str(tmp_path / "w.npy"), **kw), [0])


def test_multi_entry_points_validate_before_any_device_work():
    lib = sw._lib.load()
    ok, P = ctypes.byref(sw.SwParams.make(3)), ctypes.c_void_p(8)      # P: non-NULL, never dereferenced
    roll = lib.sw_ars_rollouts_multi_f64
    #            p   S  N  H  policy deltas nu   mean inv_std returns moments status stream
    # (every call below fails a check: none reaches a launch)
    assert roll(None, 2, 1, 5, P, P, 0.01, None, None, P, None, None, None) == 1
    assert roll(ok, 0, 1, 5, P, P, 0.01, None, None, P, None, None, None) == 3
    assert roll(ok, 2, 0, 5, P, P, 0.01, None, None, P, None, None, None) == 3
    assert roll(ok, 2, 1, -1, P, P, 0.01, None, None, P, None, None, None) == 3
    assert roll(ok, 65536, 1, 5, P, P, 0.01, None, None, P, None, None, None) == 3
    assert roll(ok, 2, 1, 5, None, P, 0.01, None, None, P, None, None, None) == 1
    assert roll(ok, 2, 1, 5, P, None, 0.01, None, None, P, None, None, None) == 1
    assert roll(ok, 2, 1, 5, P, P, 0.01, None, None, None, None, None, None) == 1
    assert roll(ok, 2, 1, 5, P, P, 0.01, P, None, P, None, None, None) == 1           # mean without inv_std
    assert roll(ok, 2, 1, 5, P, P, 0.01, None, P, P, None, None, None) == 1
    assert roll(ctypes.byref(sw.SwParams.make(9)), 2, 1, 5, P, P, 0.01, None, None, P, None, None, None) == 2
    assert roll(ctypes.byref(sw.SwParams.make(3, l_i=-1.0)), 2, 1, 5, P, P, 0.01, None, None, P, None, None,
                None) == 4
    upd = lib.sw_ars_update_multi_f64
    #           p   S  N  returns deltas policy alpha b   top_b moments rows running n_new mean inv_std sigma stream
    assert upd(None, 2, 1, P, P, P, 0.01, 1.0, 0, None, 0, None, 0, None, None, None, None) == 1
    assert upd(ok, 0, 1, P, P, P, 0.01, 1.0, 0, None, 0, None, 0, None, None, None, None) == 3
    assert upd(ok, 2, 0, P, P, P, 0.01, 1.0, 0, None, 0, None, 0, None, None, None, None) == 3
    assert upd(ok, 2, 1, None, P, P, 0.01, 1.0, 0, None, 0, None, 0, None, None, None, None) == 1
    assert upd(ok, 2, 1, P, P, None, 0.01, 1.0, 0, None, 0, None, 0, None, None, None, None) == 1
    assert upd(ok, 2, 1, P, P, P, 0.01, 1.0, 0, None, 1, P, 10, P, P, None, None) == 1   # running without moments
    assert upd(ok, 2, 1, P, P, P, 0.01, 1.0, 0, P, 1, P, -1, P, P, None, None) == 3
