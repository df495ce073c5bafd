"""Safe ARS rollouts gated on an ensemble of simulators, on the GPU: sw_safe_ars_rollouts_ensemble_f64 bit for bit
against the lane form of sw_safe_ars_rollouts_multi_f64 run once per member, against the NumPy restatement
(tests/safe_ensemble_oracle.py) on the conditioned cases, and the host layer (safe_ars.ARSBatch with sim_ensembles,
safe_ars.experiment.run_ensemble) against the kernels driven by hand."""
import os

import numpy as np
import pytest
import torch

import swimmer_amd as sw
from conftest import GOLDEN, observed
from swimmer_amd.safe_ars import experiment

import safe_ensemble_cases as cases
from test_safe_experiment_gpu import COSTS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX, ABS = sw._lib.COST_MAX_ABS_THETADOT, sw._lib.COST_ABS_OBS
LANE = sw._lib.FLAG_ROLLOUT_LANE
GUARD = 64                     # elements of guard in front of and behind every output
F64_OUT, I32_OUT = ("returns", "cost_trace", "cost_max", "worst_max"), ("first_refused", "violations", "status")
SHARED = ("returns", "cost_trace", "cost_max", "first_refused", "violations", "status")     # the single launch has them
ALL = F64_OUT + I32_OUT + ("refusing_members",)


def dv(x):
    return torch.as_tensor(x, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


class Outputs(object):
    """Every output of a launch inside a buffer of guard values; `leave_out`: those handed over as NULL."""

    def __init__(self, A, R, H, names=ALL, leave_out=()):
        self.buf, self.t = {}, {}
        for name in names:
            if name in leave_out:
                continue
            dtype = torch.float64 if name in F64_OUT else torch.int64 if name == "refusing_members" else torch.int32
            shape = (H, A, R) if name == "cost_trace" else (A, R)
            size = int(np.prod(shape))
            self.buf[name] = torch.full((size + 2 * GUARD,), -7, dtype=dtype, device=DEV)
            self.t[name] = self.buf[name][GUARD:GUARD + size].view(shape)

    def guards_stand(self):
        return all(bool((b[:GUARD] == -7).all() and (b[-GUARD:] == -7).all()) for b in self.buf.values())

    def __getitem__(self, name):
        return self.t[name]


def ensemble_launch(c, H, sims=None, leave_out=(), p=None):
    A, R = 3, 2 * c["deltas"].shape[1]
    out = Outputs(A, R, H, leave_out=leave_out)
    sw.kernels.safe_ars_rollouts_ensemble(p or c["p"], H, dv(c["policy"]), dv(c["deltas"]), c["nu"], dv(c["gated"]),
                                          dv(np.ascontiguousarray(c["sims"] if sims is None else sims)),
                                          dv(c["sim_thresh"]), dv(c["real_thresh"]), c["kind"], c["index"], **out.t)
    assert out.guards_stand()
    return out


def single_launch(c, H, sim):
    """sw_safe_ars_rollouts_multi_f64 in the lane form with one simulator [3, 3] per agent."""
    A, R = 3, 2 * c["deltas"].shape[1]
    out = Outputs(A, R, H, names=SHARED)
    p = sw.SwParams.make(c["p"].n, c["p"].l_i, c["p"].m_i, c["p"].k, flags=LANE)
    sw.kernels.safe_ars_rollouts_multi(p, H, dv(c["policy"]), dv(c["deltas"]), c["nu"], dv(c["gated"]),
                                       dv(np.ascontiguousarray(sim)), dv(c["sim_thresh"]), dv(c["real_thresh"]),
                                       c["kind"], c["index"], **out.t)
    assert out.guards_stand()
    return out


def check_equivalence(c, H):
    """The rollouts of one policy share their trajectory until the first refusal, so the ensemble's rollout is the run
    of any member that refuses first."""
    E, tag = c["sims"].shape[1], (c["p"].n, c["deltas"].shape[1], c["sims"].shape[1], H, c["kind"], c["index"])
    got = ensemble_launch(c, H)
    per = [single_launch(c, H, c["sims"][:, e]) for e in range(E)]
    first_e = torch.stack([m["first_refused"] for m in per])                  # [E, 3, R]
    first = first_e.min(dim=0).values
    assert torch.equal(got["first_refused"], first), tag
    binds = first_e == first[None]                                              # the minimising members
    shifts = torch.arange(E, dtype=torch.int64, device=DEV)[:, None, None]
    mask = torch.where(first < H, (binds.to(torch.int64) << shifts).sum(dim=0), torch.zeros_like(first, dtype=torch.int64))
    gated = [a for a in range(3) if c["gated"][a]]
    assert torch.equal(got["refusing_members"][gated], mask[gated]), tag
    for name in SHARED:
        if name == "first_refused":
            continue
        for e in range(E):
            same = bits(got[name]) == bits(per[e][name])
            where = binds[e][None] if name == "cost_trace" else binds[e]
            assert bool((same | ~where)[..., gated, :].all()), (tag, name, e)
    worst, thr = got["worst_max"], dv(c["sim_thresh"])[:, None]
    assert bool((worst[gated] <= thr[gated]).all()) and bool((worst[gated] >= 0).all()), tag
    assert bool((worst[gated][first[gated] == 0] == 0).all()), tag
    # the ungated agent: the bits of its lane-form run, in whichever member's launch
    for name in SHARED:
        assert torch.equal(bits(got[name])[..., 1, :], bits(per[0][name])[..., 1, :]), (tag, name)
    assert bool((got["first_refused"][1] == H).all()) and bool(torch.isnan(worst[1]).all()), tag
    assert bool((got["refusing_members"][1] == 0).all()), tag


@pytest.mark.parametrize("H", [0, 1, 51])
@pytest.mark.parametrize("E,n_dir", [(1, 33), (2, 17), (3, 9), (5, 5), (8, 5), (33, 1), (64, 2)])
def test_the_ensemble_rollout_is_the_run_of_the_member_that_refuses_first(E, n_dir, H):
    """n = 3, every group size 1..64 (E = 3, 5 and 33 wrap their members over the group), 66 rollouts of 64 slots, 34 of
    32, a ragged last workgroup at E = 3, 5 and 8, one rollout per wave at E = 33 and 64; all five costs."""
    for cost in COSTS:
        check_equivalence(cases.ensemble_case(3, n_dir, E, cost), H)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
def test_every_instantiation_runs(n):
    for cost in (COSTS[0], (ABS, 2 * n + 1, (0.3, 0.4), 0.004)):      # the last segment's angular speed
        check_equivalence(cases.ensemble_case(n, 3, 3, cost), 21)


@pytest.mark.parametrize("n,flags", [(3, 0), (3, LANE), (3, sw._lib.FLAG_ROLLOUT_QUAD), (6, 0)])
def test_one_simulator_or_copies_of_it_give_the_single_launchs_bits(n, flags):
    """E = 1 and E = 4 copies of one simulator: every output the two entry points share has the bits of the lane form in
    that simulator, whatever SW_FLAG_ROLLOUT_* says; worst_max and the mask agree with them."""
    H = 51
    for cost in (COSTS[0], COSTS[4] if n == 3 else (ABS, 2 * n + 1, (0.3, 0.4), 0.004)):
        c = cases.ensemble_case(n, 9, 1, cost)
        want = single_launch(c, H, c["sim"])
        p = sw.SwParams.make(n, 1.0, 1.0, 10.0, flags=flags)
        for E in (1, 4):
            got = ensemble_launch(c, H, sims=np.repeat(c["sims"], E, axis=1), p=p)
            for name in SHARED:
                assert torch.equal(bits(got[name]), bits(want[name])), (n, flags, E, name)
            refused = want["first_refused"][[0, 2]] < H
            assert torch.equal(got["refusing_members"][[0, 2]] == (1 << E) - 1, refused)
            assert torch.equal(got["refusing_members"][[0, 2]] == 0, ~refused)
            if n == 3:           # (tests/test_safe_experiment_gpu.py holds this case to refusing some and not others)
                assert bool(refused.any()) and bool((~refused).any())


def test_the_order_of_the_members_permutes_the_mask_and_nothing_else():
    H, E = 51, 5
    perm = np.array([3, 0, 4, 1, 2])               # new member j is old member perm[j]
    for cost in (COSTS[0], COSTS[4]):
        c = cases.ensemble_case(3, 9, E, cost)
        a, b = ensemble_launch(c, H), ensemble_launch(c, H, sims=c["sims"][:, perm])
        for name in F64_OUT + I32_OUT:
            assert torch.equal(bits(a[name]), bits(b[name])), name
        moved = torch.zeros_like(a["refusing_members"])
        for j, e in enumerate(perm):
            moved |= ((a["refusing_members"] >> int(e)) & 1) << j
        assert torch.equal(b["refusing_members"], moved)
        proper = (moved != 0) & (moved != (1 << E) - 1)
        assert bool(proper.any())                    # some members refuse and others do not: the permutation shows


def test_each_optional_output_may_be_null():
    H = 51
    c = cases.ensemble_case(3, 9, 5, COSTS[0])
    full = ensemble_launch(c, H)
    optional = [name for name in ALL if name != "returns"]
    for leave_out in [(name,) for name in optional] + [tuple(optional)]:
        got = ensemble_launch(c, H, leave_out=leave_out)
        for name in ALL:
            if name not in leave_out:
                assert torch.equal(bits(got[name]), bits(full[name])), (leave_out, name)


@pytest.mark.parametrize("E,bad", [(5, (2, 4)), (1, (0,)), (64, (63,)), (33, (0, 32))])
def test_a_bad_member_fails_its_agent_alone(E, bad):
    """m_i = 0 in some members of agent 0: SW_STATUS_PARAM, NaN returns, cost trace, maximum and worst_max,
    first_refused 0, no violations, the bad members' bits; the other agents keep their bits."""
    H = 21
    c = cases.ensemble_case(3, 5, E, COSTS[4])
    clean = ensemble_launch(c, H)
    sims = c["sims"].copy()
    sims[0, list(bad), 1] = 0.0
    got = ensemble_launch(c, H, sims=sims)
    for name in ALL:
        assert torch.equal(bits(got[name])[..., 1:, :], bits(clean[name])[..., 1:, :]), name
    assert bool((got["status"][0] == sw._lib.STATUS_PARAM).all())
    for name in F64_OUT:
        assert bool(torch.isnan(got[name][..., 0, :]).all()), name
    assert bool((got["first_refused"][0] == 0).all()) and bool((got["violations"][0] == 0).all())
    want = torch.zeros((), dtype=torch.int64, device=DEV)
    for e in bad:
        want |= torch.ones((), dtype=torch.int64, device=DEV) << e
    assert bool((got["refusing_members"][0] == want).all())


# ---- against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_cost", (0, 1), ids=("max_abs_thetadot", "abs_obs_3"))
@pytest.mark.parametrize("E", (3, 5))
def test_against_the_oracle(E, k_cost):
    """The conditioned cases (tests/test_safe_ars_ensemble_cpu.py holds every gate decision more than 1e-6 from its
    threshold): the discrete outcomes are the oracle's, worst_max and cost_max within 1e-9 absolute, this project's bar
    for costs against the oracle (floor["costs"] of tests/test_safe_experiment_gpu.py)."""
    H = 51
    c, want = cases.ensemble_case(3, 9, E, cases.CONDITIONED[k_cost]), cases.want(3, 9, E, k_cost, H)
    got = {name: t.cpu().numpy() for name, t in ensemble_launch(c, H).t.items()}
    err = {"worst_max": float(np.abs(got["worst_max"][[0, 2]] - want["worst_max"][[0, 2]]).max()),
           "cost_max": float(np.abs(got["cost_max"] - want["cost_max"]).max()),
           "cost_trace": float(np.abs(got["cost_trace"] - want["costs"]).max()),
           "returns": float(np.abs(got["returns"] - want["R"]).max())}
    observed(f"safe_ars_ensemble_vs_oracle_E{E}_cost{k_cost}", err)
    assert err["worst_max"] <= 1e-9 and err["cost_max"] <= 1e-9, err
    assert np.array_equal(got["first_refused"], want["first_refused"])
    assert np.array_equal(got["refusing_members"], want["refusing"])
    assert np.array_equal(got["violations"], want["violations"])
    assert np.isnan(got["worst_max"][1]).all() and not got["status"].any()
    admitted = got["first_refused"][[0, 2]] > 0
    assert admitted.any() and np.all(got["worst_max"][[0, 2]][admitted] <= c["sim_thresh"][[0, 2], None].repeat(18, 1)[admitted])


# ---- the host layer --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "safe_experiment.npz"), allow_pickle=False)


def test_a_batch_with_ensembles_is_the_kernels_driven_by_hand():
    """Three agents (ensemble, basic, ensemble) over 3 iterations, N = 4, H = 51: row a of ARSBatch(sim_ensembles=...)
    is bit for bit a loop of SeedStreams, kernels.safe_ars_rollouts_ensemble and kernels.ars_update_multi;
    member_refusals are the bit counts of refusing_members."""
    from swimmer_amd.ars.agent_batch import SeedStreams
    n_iter, N, b, H, E, alpha, nu = 3, 4, 2, 51, 5, 0.02, 0.4
    R = 2 * N
    c = cases.ensemble_case(3, N, E, COSTS[0])
    real = sw.SwimmerEnv("RealWorld", n=3)
    ens = [None if not c["gated"][a] else [tuple(row) for row in c["sims"][a]] for a in range(3)]
    ens[2] = [sw.SwimmerEnv("Simulator", n=3, l_i=row[0], m_i=row[1], k=row[2]) for row in c["sims"][2]]
    batch = sw.safe_ars.ARSBatch(real, [11, 11, 12], c["gated"] != 0, sw.safe_ars.MaxAbsThetaDot(), c["real_thresh"],
                                 c["sim_thresh"], sim_ensembles=ens)
    batch.train(n_iter, N, b, alpha, nu, H, costs="all")
    assert batch.worst_max.shape == (3, n_iter * R) and batch.refusing_members.shape == (3, n_iter * R)
    assert batch.refusing_members.dtype == np.int64 and batch.member_refusals.shape == (3, E)
    counts = ((batch.refusing_members[:, :, None] >> np.arange(E)) & 1).sum(axis=1)
    assert np.array_equal(batch.member_refusals, counts)
    assert batch.member_refusals[[0, 2]].sum() > 0 and not batch.member_refusals[1].any()
    assert np.array_equal(batch.refusing_members != 0, batch.first_refused < H)

    streams = SeedStreams(batch.seeds)
    policy = torch.zeros((3, 2, 8), dtype=torch.float64, device=DEV)
    sims = dv(np.where(np.array(c["gated"], dtype=bool)[:, None, None], c["sims"], [[[1.0, 1.0, 10.0]]]))
    assert np.array_equal(batch.sims, sims.cpu().numpy())
    for it in range(n_iter):
        deltas = dv(streams.fill(np.empty((3, N, 2, 8))))
        out = Outputs(3, R, H)
        sw.kernels.safe_ars_rollouts_ensemble(batch.params, H, policy, deltas, nu, dv(c["gated"]), sims,
                                              dv(c["sim_thresh"]), dv(c["real_thresh"]), MAX, 0, **out.t)
        sw.kernels.ars_update_multi(batch.params, out["returns"], deltas, policy, alpha, float(b), top_b=b)
        cut = slice(it * R, (it + 1) * R)
        assert np.array_equal(batch.curves[:, it], [np.mean(r) for r in out["returns"].cpu().numpy()]), it
        assert np.array_equal(batch.first_refused[:, cut], out["first_refused"].cpu().numpy()), it
        assert np.array_equal(batch.cost_max[:, cut], out["cost_max"].cpu().numpy()), it
        assert np.array_equal(batch.worst_max[:, cut], out["worst_max"].cpu().numpy(), equal_nan=True), it
        assert np.array_equal(batch.refusing_members[:, cut], out["refusing_members"].cpu().numpy()), it
        assert np.array_equal(batch.costs[:, cut], out["cost_trace"].cpu().numpy().transpose(1, 2, 0)), it
    assert np.array_equal(batch.policy, policy.cpu().numpy())


def test_run_ensemble_keeps_the_scripts_two_agents_and_stays_inside(g):
    """At the fixture's size: the basic and the single-simulator rows are run(..., rollout_kernel="lane") bit for bit,
    and the worst member of the ensemble agents never left the threshold."""
    n, n_iter, N, b, H, n_seeds, _ = (int(x) for x in g["c_cfg"])
    alpha, nu, thresh, epsilon = g["c_hyper"]
    seeds, theta_sim = g["c_seeds"].tolist(), g["c_theta_sim"]
    state = np.random.get_state()
    want = experiment.run(epsilon, thresh, n_iter, H, N, b, alpha, nu, n_seeds, seeds=seeds, theta_sim=theta_sim,
                          rollout_kernel="lane")
    out = experiment.run_ensemble(epsilon, thresh, n_iter, H, N, b, alpha, nu, n_seeds, 8, seeds=seeds,
                                  theta_sim=theta_sim, ensemble_seed=1)
    assert np.array_equal(np.random.get_state()[1], state[1])           # given seeds and theta_sim draw nothing
    for key in want:
        if key not in ("batch", "seeds"):
            assert np.array_equal(out[key], want[key], equal_nan=True), key
    assert out["seeds"] == want["seeds"]
    assert out["ensemble_returns"].shape == (n_seeds, n_iter) and out["ensemble_costs"].shape == (n_seeds, 2 * n_iter * H)
    assert out["ensemble_violations"].shape == (n_seeds,) and out["member_refusals"].shape == (n_seeds, 8)
    assert np.array_equal(out["members"], experiment.ensemble_members(theta_sim, epsilon, 8, 1))
    assert np.array_equal(out["batch"].sims[2], out["members"][:, [1, 0, 2]])        # (m_i, l_i, k) -> (l_i, m_i, k)
    assert np.array_equal(out["batch"].sims[1], np.tile(out["members"][0, [1, 0, 2]], (8, 1)))
    assert out["worst_margin"] >= 0
    observed("safe_ars_run_ensemble", {"worst_margin": out["worst_margin"],
                                       "member_refusals": out["member_refusals"].tolist(),
                                       "ensemble_violations": out["ensemble_violations"].tolist(),
                                       "safe_violations": out["safe_violations"].tolist()})
