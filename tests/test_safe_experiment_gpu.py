"""safe_ars/experiment.py as one batch, on the GPU: sw_safe_ars_rollouts_multi_f64, safe_ars.ARSBatch and
safe_ars.experiment against the reference fixture (tests/golden/safe_experiment.npz), against the single-agent kernels
bit for bit, agent by agent, and where the gate refuses everything."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import swimmer_amd as sw
from swimmer_amd.safe_ars import experiment
from conftest import GOLDEN, observed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX, ABS = sw._lib.COST_MAX_ABS_THETADOT, sw._lib.COST_ABS_OBS
# (kind, index, sim thresholds of the gated agents 0 and 2, margin of the real threshold): the reference's cost, and
# |obs[j]| on Gdot_x, Gdot_y, an angle (it starts at pi / 2) and an angular speed
# (Gdot stays tiny over 51 steps from rest: 1e-6 and 1e-5)
COSTS = [(MAX, 0, (0.45, 0.6), 0.004), (ABS, 0, (1e-6, 2e-6), 1e-8), (ABS, 1, (2e-5, 4e-5), 1e-7),
         (ABS, 4, (1.575, 1.58), 0.0005), (ABS, 3, (0.3, 0.4), 0.004)]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "safe_experiment.npz"), allow_pickle=False)


def fixture_envs(g):
    tr, ts = g["a_theta_real"], g["a_theta_sim"]
    return (sw.SwimmerEnv("RealWorld", n=3, m_i=tr[0], l_i=tr[1], k=tr[2]),
            sw.SwimmerEnv("Simulator", n=3, m_i=ts[0], l_i=ts[1], k=ts[2]))


def fixture_batch(g, agents=None, **kw):
    """The fixture's four agents (seed 3 basic, seed 3 safe, seed 4 basic, seed 4 safe), or some of them."""
    real, sim = fixture_envs(g)
    seeds = [int(s) for s in g["a_seeds"] for _ in range(2)]
    gated = [False, True] * len(g["a_seeds"])
    agents = range(len(seeds)) if agents is None else agents
    thresh, sim_thresh = g["a_hyper"][2:4]
    return sw.safe_ars.ARSBatch(real, [seeds[a] for a in agents], [gated[a] for a in agents],
                                sw.safe_ars.MaxAbsThetaDot(), thresh, sim_thresh, sim, **kw)


@pytest.fixture(scope="module")
def trained(g):
    """The four agents trained as one batch with the fixture's configuration (shared, never modified)."""
    n, n_iter, N, b, H = (int(x) for x in g["a_cfg"])
    alpha, nu = g["a_hyper"][:2]
    batch = fixture_batch(g)
    batch.train(n_iter, N, b, alpha, nu, H, costs="reference")
    return batch


def test_batch_and_experiment_against_the_reference(g, trained):
    """Discrete outcomes equal the reference's; curves, final policies and cost traces are within 4x the error the
    single-agent Basic_ARS.train / Safe_ARS.train have on the same fixture (the factor covers the device update's
    other order of summation), or within the bars tests/test_hip_parity.py holds those classes to."""
    n, n_iter, N, b, H = (int(x) for x in g["a_cfg"])
    alpha, nu, thresh, sim_thresh = g["a_hyper"]
    real, sim = fixture_envs(g)
    kinds = ["unsafe", "safe"] * len(g["a_seeds"])
    want = {key: np.array([g[f"a_{kinds[a]}_{key}"][a // 2] for a in range(4)])
            for key in ("returns", "policy", "costs", "cost_max")}
    # the parent's route: one agent at a time on NumPy's global generator
    single = {"returns": [], "policy": [], "costs": []}
    state = np.random.get_state()
    try:
        for a in range(4):
            agent = sw.safe_ars.Safe_ARS(sw.safe_ars.MaxAbsThetaDot(), thresh, sim_thresh, sim) if a % 2 \
                else sw.safe_ars.Basic_ARS()
            np.random.seed(int(g["a_seeds"][a // 2]))
            with contextlib.redirect_stdout(io.StringIO()):
                curve, states = agent.train(n_iter, real, N, b, alpha, nu, H)
            single["returns"].append(curve)
            single["policy"].append(agent.policy)
            single["costs"].append(np.abs(states[:2 * n_iter, :, 3::2]).max(axis=2).reshape(-1))
    finally:
        np.random.set_state(state)
    got = {"returns": trained.curves, "policy": trained.policy, "costs": trained.costs}
    floor = {"returns": 1e-12 * np.maximum(1.0, np.abs(want["returns"])).max(), "policy": 1e-9, "costs": 1e-9}
    figures = {}
    for key in ("returns", "policy", "costs"):
        e_single = float(np.abs(np.array(single[key]) - want[key]).max())
        e_batch = float(np.abs(got[key] - want[key]).max())
        figures[key] = {"single_agent": e_single, "batch": e_batch, "bound": max(4 * e_single, floor[key])}
    observed("safe_experiment_batch_vs_reference", figures)
    for key, f in figures.items():
        assert f["batch"] <= f["bound"], (key, f)
    # discrete outcomes
    assert np.array_equal(trained.first_refused[1::2], g["a_safe_first_refused"])
    assert np.all(trained.first_refused[0::2] == H)
    assert np.array_equal(trained.real_violations[1::2], g["a_safe_violations"])
    assert np.all(trained.status == 0)
    assert np.abs(trained.cost_max - want["cost_max"]).max() <= max(4 * figures["costs"]["single_agent"], 1e-9)
    # the basic agents' violations are not printed by the reference: counted from its own costs (every basic
    # rollout's maximum is further than 1e-6 from the threshold, so the count's sign test cannot flip)
    assert np.abs(want["cost_max"][0::2] - thresh).min() > 1e-6
    assert np.all(trained.real_violations[0::2] > 0)

    # experiment.run from the script's use of the global generator (the fixture's second block)
    n, n_iter, N, b, H, n_seeds, global_seed = (int(x) for x in g["c_cfg"])
    alpha, nu, thresh, epsilon = g["c_hyper"]
    try:
        np.random.seed(global_seed)
        out = experiment.run(epsilon, thresh, n_iter, H, N, b, alpha, nu, n_seeds)
        assert np.random.randint(2**32 - 1) == int(g["c_next_draw"])
    finally:
        np.random.set_state(state)
    assert np.array_equal(out["theta_sim"], g["c_theta_sim"]) and out["seeds"] == g["c_seeds"].tolist()
    assert out["mean_safe_returns"].shape == (n_iter,) and out["mean_safe_costs"].shape == (2 * n_iter * H,)
    assert out["std_unsafe_returns"].shape == (n_iter,)
    means = {}
    for kind in ("unsafe", "safe"):
        for key, bar in (("returns", figures["returns"]["bound"]), ("costs", figures["costs"]["bound"])):
            err = float(np.abs(out[f"mean_{kind}_{key}"] - g[f"c_mean_{kind}_{key}"]).max())
            means[f"mean_{kind}_{key}"] = err
            assert err <= bar, (kind, key, err, bar)
    observed("safe_experiment_run_vs_reference", means)


def bits(t):
    return t.contiguous().view(torch.int64)


def mixed_case(n, n_dir, cost, flags):
    """Three agents, gated [1, 0, 1], with three simulators and thresholds; deterministic host data."""
    kind, index, sim_thr, margin = cost
    rs = np.random.RandomState(1000 * n + n_dir)
    m, d = n - 1, 2 * n + 2
    policy = 0.6 * (2 * rs.rand(3, m, d) - 1)
    deltas = 2 * rs.rand(3, n_dir, m, d) - 1
    sim = np.array([[1.03, 0.98, 10.1], [0.9, 1.1, 9.0], [0.97, 1.04, 9.8]])          # (l_i, m_i, k)
    sim_thresh = np.array([sim_thr[0], 0.0, sim_thr[1]])
    real_thresh = sim_thresh + margin
    real_thresh[1] = sim_thr[0]                                                       # the basic agent's, for its count
    return dict(p=sw.SwParams.make(n, 1.0, 1.0, 10.0, flags=flags), policy=policy, deltas=deltas, nu=0.4,
                gated=np.array([1, 0, 1], dtype=np.int32), sim=sim, sim_thresh=sim_thresh, real_thresh=real_thresh,
                kind=kind, index=index)


def host_cost(traj, kind, index):
    """The native cost on a trajectory [H, d, B] -> [H, B], NaN as np.max propagates it."""
    if kind == MAX:
        return np.max(np.abs(traj[:, 3::2, :]), axis=1)
    return np.abs(traj[:, index, :])


def check_against_single_agent_kernels(c, H):
    p, A, n_dir = c["p"], 3, c["deltas"].shape[1]
    R = 2 * n_dir
    dv = lambda x: torch.as_tensor(x, device=DEV)           # noqa: E731
    i32 = lambda: torch.full((A, R), -7, dtype=torch.int32, device=DEV)    # noqa: E731
    trace = torch.full((H, A, R), -7.0, dtype=torch.float64, device=DEV)
    cmax = torch.full((A, R), -7.0, dtype=torch.float64, device=DEV)
    first, viol, status = i32(), i32(), i32()
    ret = sw.kernels.safe_ars_rollouts_multi(p, H, dv(c["policy"]), dv(c["deltas"]), c["nu"], dv(c["gated"]),
                                             dv(c["sim"]), dv(c["sim_thresh"]), dv(c["real_thresh"]), c["kind"],
                                             c["index"], cost_trace=trace, cost_max=cmax, first_refused=first,
                                             violations=viol, status=status)
    for a in range(A):
        pols = np.empty((R,) + c["policy"].shape[1:])
        pols[0::2] = c["policy"][a] + c["nu"] * c["deltas"][a]
        pols[1::2] = c["policy"][a] - c["nu"] * c["deltas"][a]
        traj = torch.zeros((H, p.d, R), dtype=torch.float64, device=DEV)
        st = torch.zeros(R, dtype=torch.int32, device=DEV)
        tag = (p.n, p.flags, n_dir, H, c["kind"], c["index"], a)
        if c["gated"][a]:
            fr, vi = (torch.zeros(R, dtype=torch.int32, device=DEV) for _ in range(2))
            p_sim = sw.SwParams.make(p.n, *c["sim"][a])
            want = sw.kernels.safe_rollouts(p, p_sim, H, dv(pols), c["kind"], c["index"], c["sim_thresh"][a],
                                            c["real_thresh"][a], traj=traj, first_refused=fr, violations=vi, status=st)
            assert torch.equal(first[a], fr), tag
            assert torch.equal(viol[a], vi), tag
        else:
            want = sw.kernels.rollout(p, H, dv(pols), traj=traj, status=st)
            assert torch.all(first[a] == H), tag
        assert torch.equal(bits(ret[a]), bits(want)), tag
        assert torch.equal(status[a], st), tag
        cost = host_cost(traj.cpu().numpy(), c["kind"], c["index"])
        assert np.array_equal(trace[:, a, :].cpu().numpy(), cost, equal_nan=True), tag
        assert np.array_equal(cmax[a].cpu().numpy(), cost.max(axis=0) if H else np.zeros(R), equal_nan=True), tag
        if not c["gated"][a]:
            assert np.array_equal(viol[a].cpu().numpy(), (cost > c["real_thresh"][a]).sum(axis=0)), tag
    return first.cpu().numpy()


@pytest.mark.parametrize("H", [0, 1, 51])
@pytest.mark.parametrize("n_dir", [1, 9])
def test_mirror_quad_form_has_the_single_agent_kernels_bits(n_dir, H):
    """2N = 2 (a nearly empty workgroup) and 18 (a ragged second one) of 16 slots; H = 0, 1 and 51 (the two-step
    loop's tail); both cost kinds, |obs[j]| on Gdot_x, Gdot_y, an angle and an angular speed."""
    for cost in COSTS:
        first = check_against_single_agent_kernels(mixed_case(3, n_dir, cost, 0), H)
        if H == 51 and n_dir == 9:       # the case is worth its name: the gate refuses some rollouts and not others
            gated = first[[0, 2]]
            assert (gated < H).any() and (gated == H).any(), (cost, first)


@pytest.mark.parametrize("H", [0, 1, 51])
def test_lane_form_has_the_single_agent_kernels_bits(H):
    """2N = 66 of 64 slots per workgroup, n = 3 in the lane form."""
    for cost in COSTS:
        first = check_against_single_agent_kernels(mixed_case(3, 33, cost, sw._lib.FLAG_ROLLOUT_LANE), H)
        if H == 51:
            gated = first[[0, 2]]
            assert (gated < H).any() and (gated == H).any(), (cost, first)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
def test_every_lane_instantiation_runs(n):
    """One rollout per lane for every n = 2..8 (n = 4..8 have no other form here)."""
    for cost in (COSTS[0], (ABS, 2 * n + 1, (0.3, 0.4), 0.004)):      # the last segment's angular speed
        check_against_single_agent_kernels(mixed_case(n, 3, cost, sw._lib.FLAG_ROLLOUT_LANE), 21)


def all_outputs(c, H):
    """Every output of one sw_safe_ars_rollouts_multi_f64 launch of a mixed_case, as int64 / int32 tensors."""
    A, R = 3, 2 * c["deltas"].shape[1]
    dv = lambda x: torch.as_tensor(x, device=DEV)           # noqa: E731
    i32 = lambda: torch.full((A, R), -7, dtype=torch.int32, device=DEV)    # noqa: E731
    trace = torch.full((H, A, R), -7.0, dtype=torch.float64, device=DEV)
    cmax = torch.full((A, R), -7.0, dtype=torch.float64, device=DEV)
    first, viol, status = i32(), i32(), i32()
    ret = sw.kernels.safe_ars_rollouts_multi(c["p"], H, dv(c["policy"]), dv(c["deltas"]), c["nu"], dv(c["gated"]),
                                             dv(c["sim"]), dv(c["sim_thresh"]), dv(c["real_thresh"]), c["kind"],
                                             c["index"], cost_trace=trace, cost_max=cmax, first_refused=first,
                                             violations=viol, status=status)
    return bits(ret), bits(trace), bits(cmax), first, viol, status


@pytest.mark.parametrize("n,n_dir", [(4, 9), (3, 1366)], ids=["n4-no-row-form", "n3-no-quad-form"])
def test_a_form_without_a_kernel_hands_over_to_the_lane_form(n, n_dir):
    """Where the plan of the launch names a form that has no safe-ARS kernel -- the row form at n = 4 (18 rollouts per
    agent: a full and a partial 16-slot group), the quad form at n = 3 with 3 x 2736 slots, more than the mirror-quad
    form's 8192 -- the launch runs in the lane form: the bits of the same call under FLAG_ROLLOUT_LANE.  H = 5: a
    four-step trip and a remainder in the forms that are not taken."""
    cost = (ABS, 2 * n + 1, (0.3, 0.4), 0.004)
    auto = all_outputs(mixed_case(n, n_dir, cost, 0), 5)
    lane = all_outputs(mixed_case(n, n_dir, cost, sw._lib.FLAG_ROLLOUT_LANE), 5)
    for got, want in zip(auto, lane):
        assert torch.equal(got, want), (n, n_dir)
    assert (auto[3] >= 0).all() and (auto[5] == 0).all()          # every rollout was run: first_refused, status written


def test_an_agent_of_a_batch_is_the_agent_alone(g):
    """Row a of a batch of four after three training iterations, bit for bit the batch of that agent alone; both
    ways of keeping costs."""
    n, n_iter, N, b, H = (int(x) for x in g["a_cfg"])
    alpha, nu = g["a_hyper"][:2]
    whole = fixture_batch(g)
    whole.train(3, N, b, alpha, nu, H, costs="all")
    assert whole.costs.shape == (4, 3 * 2 * N, H)
    for a in range(4):
        alone = fixture_batch(g, agents=[a])
        alone.train(3, N, b, alpha, nu, H, costs="all")
        for key in ("policy", "curves", "costs", "cost_max", "first_refused", "real_violations", "status"):
            assert np.array_equal(getattr(whole, key)[a], getattr(alone, key)[0], equal_nan=True), (a, key)
        ref = fixture_batch(g, agents=[a])
        ref.train(3, N, b, alpha, nu, H, costs="reference")
        assert np.array_equal(ref.costs[0], whole.costs[a, :6].reshape(-1))
        assert np.array_equal(ref.policy, alone.policy)
        assert np.array_equal(whole.cost_max[a], whole.costs[a].max(axis=1))


def test_refusals_stay_with_their_agent(g):
    """A simulator that breaks the parameter rule fails alone; a NaN simulator threshold refuses at step 0; the basic
    agent next to them trains on."""
    n, n_iter, N, b, H = (int(x) for x in g["a_cfg"])
    alpha, nu, thresh, sim_thresh = g["a_hyper"]
    real, sim = fixture_envs(g)
    broken = sw.SwimmerEnv("Simulator", n=3, m_i=1.0, l_i=-1.0, k=10.0)
    seed = int(g["a_seeds"][0])
    batch = sw.safe_ars.ARSBatch(real, [seed] * 3, [True, True, False], sw.safe_ars.MaxAbsThetaDot(), thresh,
                                 [sim_thresh, float("nan"), 0.0], [broken, sim, None])
    batch.train(3, N, b, alpha, nu, H, costs="all")
    assert batch.status.tolist() == [8, 0, 0]                     # SW_STATUS_PARAM
    assert np.isnan(batch.curves[0]).all() and np.isnan(batch.costs[0]).all() and np.isnan(batch.cost_max[0]).all()
    assert np.all(batch.first_refused[:2] == 0) and np.all(batch.real_violations[:2] == 0)
    assert np.all(batch.curves[1] == 0.0) and np.all(batch.costs[1] == 0.0)      # the reset state's cost, H times
    alone = fixture_batch(g, agents=[0])
    alone.train(3, N, b, alpha, nu, H, costs="all")
    for key in ("policy", "curves", "costs", "cost_max", "first_refused", "real_violations"):
        assert np.array_equal(getattr(batch, key)[2], getattr(alone, key)[0]), key
    assert np.isfinite(batch.curves[2]).all() and np.all(batch.first_refused[2] == H)


def test_training_loop_equals_the_plain_synchronous_loop(g):
    """train() keeps four host buffers of deltas in flight, ten iterations of results on the device and a ring of
    cost traces; 23 iterations wrap every ring.  The same kernels driven one iteration at a time with fresh buffers and
    a host read after each give the same bits."""
    n, _, N, b, _ = (int(x) for x in g["a_cfg"])
    alpha, nu = g["a_hyper"][:2]
    n_iter, H, R = 23, 20, 2 * N
    batch = fixture_batch(g)
    batch.train(n_iter, N, b, alpha, nu, H, costs="all")
    ref = fixture_batch(g)
    ref.train(n_iter, N, b, alpha, nu, H, costs="reference")
    assert np.array_equal(ref.costs, batch.costs[:, :2 * n_iter].reshape(4, -1))
    assert np.array_equal(ref.policy, batch.policy) and np.array_equal(ref.curves, batch.curves)

    from swimmer_amd.ars.agent_batch import SeedStreams
    dv = lambda x: torch.as_tensor(x, device=DEV)           # noqa: E731
    streams = SeedStreams(batch.seeds)
    policy = torch.zeros((4, 2, 8), dtype=torch.float64, device=DEV)
    gated, sim = dv(batch.gated.astype(np.int32)), dv(batch.sim)
    sim_thr, real_thr = dv(batch.sim_thresh), dv(batch.real_thresh)
    for it in range(n_iter):
        deltas = dv(streams.fill(np.empty((4, N, 2, 8))))
        trace = torch.zeros((H, 4, R), dtype=torch.float64, device=DEV)
        first = torch.zeros((4, R), dtype=torch.int32, device=DEV)
        ret = sw.kernels.safe_ars_rollouts_multi(batch.params, H, policy, deltas, nu, gated, sim, sim_thr, real_thr,
                                                 MAX, 0, cost_trace=trace, first_refused=first)
        sw.kernels.ars_update_multi(batch.params, ret, deltas, policy, alpha, float(b), top_b=b)
        rets = ret.cpu().numpy()
        assert np.array_equal(batch.curves[:, it], [np.mean(r) for r in rets]), it
        assert np.array_equal(batch.first_refused[:, it * R:(it + 1) * R], first.cpu().numpy()), it
        assert np.array_equal(batch.costs[:, it * R:(it + 1) * R], trace.cpu().numpy().transpose(1, 2, 0)), it
    assert np.array_equal(batch.policy, policy.cpu().numpy())
