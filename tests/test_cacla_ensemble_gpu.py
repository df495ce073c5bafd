"""CACLA gated on an ensemble of simulators (sw_cacla_safe_ensemble_run_f64) on the GPU: parity with
tests/cacla_ensemble_oracle.py on the cases of tests/cacla_ensemble_cases.py, one member and copies of one simulator
against the single-simulator kernel bit for bit at every instantiation, permuted members, the prefix rule against the
single-simulator kernel run once per member, the two optional records, split runs, containment of a bad member and of
a NaN threshold, and the classes.

Bounds: 1e-9 absolute against the oracle on rewards, final weights, state and worst_rec -- the project's standing bound
for runs of this length (tests/test_cacla_safe_gpu.py); masks, the NaN pattern, counters, first refusals and member
refusals equal.  Every decision of a case is at least 1e-6 from its edge in the oracle's own run
(tests/test_cacla_ensemble_cpu.py asserts it without a GPU, and the parity test again before it compares): 1e-9 of
rounding cannot flip one.  Everything else is compared bit for bit."""
import numpy as np
import pytest
import torch

import swimmer_amd as sw
from conftest import observed
from swimmer_amd import cacla
from swimmer_amd.ars.parameters import EnvParam
from swimmer_amd.cacla import safe_kernels
from swimmer_amd.safe_ars import MaxAbsThetaDot

import cacla_ensemble_cases as cases
import cacla_oracle
import test_cacla_safe_gpu as single
from test_cacla_safe_gpu import same_bits, t64

pytestmark = pytest.mark.gpu

DEV = single.DEV
GAMMA, ALPHA, SIM = single.GAMMA, single.ALPHA, single.SIM
GUARD = 7                         # guard entries on each side of worst_rec
_seen = {}


def launch(n, cost, gamma, alpha, noise, gated, sims, sim_thr, real_thr, w0, parts=None, worst=True, members=True,
           rec=True):
    """Runs of A agents through the ensemble wrapper, as one launch or split into `parts`; sims [A, E, 3].  worst /
    members / rec: whether worst_rec / member_refusals / admitted_rec are given.  -> dict of host arrays."""
    p = sw.SwParams.make(n)
    A, steps = noise.shape[0], noise.shape[1]
    sims = t64(np.asarray(sims, dtype=np.float64).reshape(A, -1, 3))
    E = sims.shape[1]
    w = t64(w0).clone()
    s = t64(np.tile(np.array(sw.SwimmerEnv(n=n).reset()), (A, 1))).clone()
    noise = t64(noise)
    last = torch.full((A,), float("nan"), dtype=torch.float64, device=DEV)
    counters = torch.zeros((A, 3), dtype=torch.int32, device=DEV)
    first = torch.full((A,), -1, dtype=torch.int32, device=DEV)
    status = torch.zeros(A, dtype=torch.int32, device=DEV)
    refusals = torch.zeros((A, E), dtype=torch.int32, device=DEV) if members else None
    args = (t64(gamma), t64(alpha))
    gate = (torch.as_tensor(np.asarray(gated, dtype=np.int32), device=DEV), sims, t64(sim_thr), t64(real_thr))
    rewards, recs, worsts, t = [], [], [], 0
    for c in (parts or [steps]):
        r = torch.empty((A, c), dtype=torch.int32, device=DEV) if rec else None
        # worst_rec between guard entries: one buffer, the kernel gets the middle of it
        buf = torch.full((A * c + 2 * GUARD,), -7.0, dtype=torch.float64, device=DEV) if worst else None
        wr = buf[GUARD:GUARD + A * c].view(A, c) if worst else None
        rewards.append(safe_kernels.cacla_safe_ensemble_run(
            p, c, t, *args, noise[:, t:t + c].contiguous(), *gate, cost.kind, cost.index, w, s, last, counters, first,
            admitted_rec=r, worst_rec=wr, member_refusals=refusals, status=status))
        if worst:
            guard = torch.cat([buf[:GUARD], buf[GUARD + A * c:]]).cpu().numpy()
            assert (guard == -7.0).all(), guard
            worsts.append(wr.clone())
        if rec:
            recs.append(r)
        t += c
    out = dict(rewards=torch.cat(rewards, dim=1).cpu().numpy(), weights=w.cpu().numpy(), state=s.cpu().numpy(),
               last=last.cpu().numpy(), counters=counters.cpu().numpy(), first=first.cpu().numpy(),
               status=status.cpu().numpy())
    if rec:
        out["admitted"] = torch.cat(recs, dim=1).cpu().numpy()
    if worst:
        out["worst"] = torch.cat(worsts, dim=1).cpu().numpy()
    if members:
        out["refusals"] = refusals.cpu().numpy()
    return out


SINGLE_KEYS = ("rewards", "admitted", "weights", "state", "last", "counters", "first", "status")


def same(a, b, keys):
    """Every output of `keys` equal as bit patterns (the doubles as 64-bit patterns, NaNs included)."""
    for key in keys:
        x, y = a[key], b[key]
        assert (same_bits(x, y) if x.dtype == np.float64 else np.array_equal(x, y)), key


# ---- (a) oracle parity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(cases.CASES))
def test_a_gated_agent_against_the_oracle(tag):
    n, kind, w, noise, sim_thr, real_thr, rows = cases.inputs(tag)
    o = cases.want(tag)
    adm = o["admitted"]
    assert adm.sum() >= 4 and (~adm).sum() >= 4, adm.sum()
    assert min(o["min_sim_margin"], o["min_real_margin"], o["min_td"]) >= 1e-6, o
    g = launch(n, single.costs(kind)[0], [GAMMA], [ALPHA], noise[None], [1], rows[None], [sim_thr], [real_thr], w[None])
    nan = np.isnan(o["rewards"])
    fig = {"rewards": float(np.abs(g["rewards"][0][~nan] - o["rewards"][~nan]).max()),
           "weights": float(np.abs(g["weights"][0] - o["weights"]).max()),
           "state": float(np.abs(g["state"][0] - o["state"]).max()),
           "worst": float(np.abs(g["worst"][0] - o["worst"]).max()),
           "members": int(len(rows)), "admitted": int(adm.sum()), "counters": [int(v) for v in o["counters"]],
           "oracle_min_sim_margin": float(o["min_sim_margin"]), "oracle_min_real_margin": float(o["min_real_margin"]),
           "oracle_min_td": float(o["min_td"])}
    print(tag, fig)
    _seen[tag] = fig
    observed("cacla_ensemble_parity", _seen)
    assert np.array_equal(g["admitted"][0].astype(bool), adm)
    assert np.array_equal(np.isnan(g["rewards"][0]), nan)
    assert tuple(g["counters"][0]) == tuple(o["counters"])
    assert g["first"][0] == (-1 if o["first_refused"] is None else o["first_refused"])
    assert np.array_equal(g["refusals"][0], o["member_refusals"])
    assert g["status"][0] == 0
    assert not np.isnan(g["worst"][0]).any()
    assert fig["rewards"] <= 1e-9 and fig["weights"] <= 1e-9 and fig["state"] <= 1e-9 and fig["worst"] <= 1e-9, fig


# ---- (b) one member is the single-simulator kernel ----------------------------------------------------------------
def mixed_rows(n, steps=100):
    """Six agents, gated and ungated rows mixed as in test_ungated_rows_are_the_plain_kernel_bit_for_bit."""
    A = 6
    gammas, alphas, sigmas = np.linspace(0.5, 0.95, A), [0.1, 0.01, 0.03] * 2, [1.0, 25.0, 0.1] * 2
    seeds, gated = list(range(40, 40 + A)), [0, 1, 0, 0, 1, 0]
    w0 = np.stack([cacla.draw_networks(n, torch.Generator().manual_seed(s)) for s in seeds])
    noise = np.stack([np.random.RandomState(s).multivariate_normal(np.zeros(n - 1), v * np.identity(n - 1), size=steps)
                      for s, v in zip(seeds, sigmas)])
    sims = np.array([SIM, SIM, (1.0, 1.0, 10.0), SIM, (0.99, 1.02, 9.8), SIM])
    return (n, MaxAbsThetaDot(), gammas, alphas, noise, gated), sims, ([0.05] * A, [0.04] * A, w0), (seeds, sigmas)


@pytest.mark.parametrize("n", range(2, 9))        # every instantiation of both kernels
def test_one_member_is_the_single_simulator_kernel_bit_for_bit(n):
    head, sims, tail, (seeds, sigmas) = mixed_rows(n)
    one = single.launch(*head, sims, *tail)
    got = launch(*head, sims[:, None], *tail)
    assert (one["counters"][[1, 4], 0] < 100).all()        # the gated rows did meet their gate
    same(got, one, SINGLE_KEYS)
    gated = np.array(head[5]) != 0
    assert np.array_equal(got["refusals"][:, 0], np.where(gated, 100 - one["counters"][:, 0], 0))
    assert np.isnan(got["worst"][~gated]).all() and not np.isnan(got["worst"][gated]).any()
    # the ungated rows are the plain kernel's
    free = np.flatnonzero(~gated)
    plain = cacla.CACLABatch(sw.SwimmerEnv(n=n), head[2], head[3], sigmas, seeds)
    r_plain = plain.run(100)
    assert plain.actor_updates[free].sum() > 0
    assert same_bits(got["rewards"][free], r_plain[free]) and same_bits(got["weights"][free], plain.weights[free])
    assert same_bits(got["state"][free], plain.state[free])
    assert np.array_equal(got["counters"][free, 2], plain.actor_updates[free])
    assert np.array_equal(got["status"][free], plain.status[free])


# ---- (c) copies of one simulator, permuted members ------------------------------------------------------------------
@pytest.mark.parametrize("E", (5, 7, 64))
@pytest.mark.parametrize("n", (3, 6))
def test_copies_of_one_simulator_are_the_single_simulator(n, E):
    head, sims, tail, _ = mixed_rows(n)
    one = single.launch(*head, sims, *tail)
    got = launch(*head, np.repeat(sims[:, None], E, axis=1), *tail)
    same(got, one, SINGLE_KEYS)
    assert got["refusals"].shape == (6, E) and (got["refusals"] == got["refusals"][:, :1]).all()
    assert got["refusals"][[1, 4]].all()


@pytest.mark.parametrize("tag", ("n3", "n6_e7", "n3_e64"))
def test_permuting_the_members_changes_only_the_order_of_member_refusals(tag):
    n, kind, w, noise, sim_thr, real_thr, rows = cases.inputs(tag)
    perm = np.roll(np.arange(len(rows))[::-1], 2)          # member 0 leaves slot 0
    assert perm[0] != 0 and sorted(perm) == list(range(len(rows)))
    args = (n, single.costs(kind)[0], [GAMMA], [ALPHA], noise[None], [1])
    a = launch(*args, rows[None], [sim_thr], [real_thr], w[None])
    b = launch(*args, rows[perm][None], [sim_thr], [real_thr], w[None])
    same(a, b, SINGLE_KEYS + ("worst",))
    assert np.array_equal(a["refusals"][0][perm], b["refusals"][0])
    assert len(set(a["refusals"][0].tolist())) > 1


# ---- (d) the prefix rule: independent of the oracle -------------------------------------------------------------------
@pytest.mark.parametrize("tag", ("n3", "n6"))
def test_the_ensemble_parts_from_its_members_at_the_first_refusal(tag):
    n, kind, w, noise, sim_thr, real_thr, rows = cases.inputs(tag)
    E = len(rows)
    cost = single.costs(kind)[0]
    ens = launch(n, cost, [GAMMA], [ALPHA], noise[None], [1], rows[None], [sim_thr], [real_thr], w[None])
    # the single-simulator kernel once per member: E agents with the same weights and noise, each in its own simulator
    per = single.launch(n, cost, [GAMMA] * E, [ALPHA] * E, np.repeat(noise[None], E, axis=0), [1] * E, rows,
                        [sim_thr] * E, [real_thr] * E, np.repeat(w[None], E, axis=0))
    assert (per["first"] >= 0).all()
    k = int(per["first"].min())
    assert k >= 1 and ens["first"][0] == k
    for e in range(E):
        assert same_bits(per["rewards"][e][:k], ens["rewards"][0][:k])
    assert not ens["admitted"][0][k] and ens["admitted"][0][:k].all()


# ---- (e) the records ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (3, 6))
def test_the_records_are_optional_and_worst_rec_sides_with_the_mask(n):
    head, _, tail, _ = mixed_rows(n)
    rows = cases.members(n, 5, 0.1)[1]
    sims = np.repeat(rows[None], 6, axis=0)
    full = launch(*head, sims, *tail)                  # worst_rec sits between guard entries (checked in launch)
    gated = np.array(head[5]) != 0
    adm, thr = full["admitted"].astype(bool), np.array(tail[0])[:, None]
    assert np.isnan(full["worst"][~gated]).all()
    assert 0 < adm[gated].sum() < adm[gated].size
    assert (full["worst"][gated] <= thr[gated])[adm[gated]].all()
    assert (full["worst"][gated] > thr[gated])[~adm[gated]].all()
    assert not full["refusals"][~gated].any() and full["refusals"][gated].all()
    for absent in (dict(worst=False), dict(members=False), dict(rec=False),
                   dict(worst=False, members=False, rec=False)):
        part = launch(*head, sims, *tail, **absent)
        same(part, full, [key for key in full if key in part])
        assert len(part) == len(full) - len(absent)


# ---- (f) splitting changes nothing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (3, 6))
def test_splitting_a_run_changes_nothing(n):
    A, steps = 3, 150
    rs = np.random.RandomState(n)
    w0 = np.stack([cacla.draw_networks(n, torch.Generator().manual_seed(s)) for s in (1, 2, 3)])
    noise = rs.normal(0.0, [[[5.0]], [[7.0]], [[10.0]]], size=(A, steps, n - 1))
    sims = np.repeat(cases.members(n, 7, 0.2)[1][None], A, axis=0)
    args = (n, MaxAbsThetaDot(), [0.9, 0.5, 0.95], [0.01, 0.003, 0.003], noise, [1, 0, 1], sims, [0.05, 0.05, 0.1],
            [0.04, 0.04, 0.08], w0)
    whole = launch(*args)
    assert not whole["status"].any() and whole["counters"][:, 2].sum() > 0
    assert 0 < whole["counters"][0, 0] < steps and 0 < whole["counters"][2, 0] < steps
    assert whole["counters"][1, 0] == steps and (whole["first"][[0, 2]] >= 0).all()
    assert whole["refusals"][[0, 2]].all() and not whole["refusals"][1].any()
    for parts in ([64, 86], [1, 149]):
        split = launch(*args, parts=parts)
        same(split, whole, list(whole))


# ---- (g) containment ----------------------------------------------------------------------------------------------------------
def test_a_bad_member_and_a_nan_threshold_stay_contained():
    n, A, steps, E = 3, 4, 96, 5
    rs = np.random.RandomState(11)
    w0 = rs.uniform(-0.3, 0.3, (A, n, cacla_oracle.net_doubles(n)))
    noise = rs.normal(0.0, 5.0, size=(A, steps, n - 1))
    sims = np.repeat(cases.members(n, E, 0.1)[1][None], A, axis=0)
    sims[1, 3] = (-1.0, 0.97, 10.3)                        # one bad member, slot 3 of 5
    sim_thr = np.array([0.05, 0.05, np.nan, 0.07])
    real_thr = np.full(A, 0.075)
    cost = MaxAbsThetaDot()
    g = launch(n, cost, [0.9] * A, [0.01] * A, noise, [1] * A, sims, sim_thr, real_thr, w0)
    s0 = np.array(sw.SwimmerEnv(n=n).reset())
    assert g["status"][1] == safe_kernels.STATUS_PARAM and g["status"][[0, 2, 3]].tolist() == [0, 0, 0]
    for a in (1, 2):                                       # every step refused: nothing moved
        assert np.isnan(g["rewards"][a]).all() and not g["admitted"][a].any()
        assert np.array_equal(g["weights"][a], w0[a]) and np.array_equal(g["state"][a], s0)
        assert g["counters"][a].tolist() == [0, 0, 0] and g["first"][a] == 0 and np.isnan(g["last"][a])
    assert (g["worst"][1] == np.inf).all() and g["refusals"][1, 3] == steps
    assert (g["refusals"][1, [0, 1, 2, 4]] < steps).all()  # the good members of that agent still give their own verdict
    assert (g["refusals"][2] == steps).all() and np.isfinite(g["worst"][2]).all()   # a NaN threshold: every member
    keep = [0, 3]
    alone = launch(n, cost, [0.9] * 2, [0.01] * 2, noise[keep], [1] * 2, sims[keep], sim_thr[keep], real_thr[keep],
                   w0[keep])
    assert 0 < alone["counters"][0, 0] < steps
    for key in g:                                          # the others have the bits of a launch without those two
        x, y = g[key][keep], alone[key]
        assert (same_bits(x, y) if x.dtype == np.float64 else np.array_equal(x, y)), key


# ---- (h) the classes ------------------------------------------------------------------------------------------------------------
def members_of(n, rows):
    return [EnvParam("member", n, 0, r[0], r[1], 1e-3, r[2], 0.0) for r in rows]


def single_ensemble(env, gamma, alpha, sigma, seed, steps, rows, cost, real_thr, sim_thr):
    torch.manual_seed(seed)
    np.random.seed(seed)
    agent = cacla.CACLA_SE_agent(gamma, alpha, sigma, None, cost, real_thr, sim_thr,
                                 sim_ensemble=members_of(env.n, rows))
    rewards = agent.run(env, steps)
    return rewards, np.concatenate([agent.actor_weights, agent.critic_weights[None]]), agent


def test_batch_rows_are_the_single_classes_bit_for_bit():
    env, steps, A, E = sw.SwimmerEnv(n=3), 100, 67, 4
    idx = np.arange(A)
    gammas = np.linspace(0.1, 0.95, A)
    alphas = np.array([0.01, 0.003, 0.001, 0.0003, 0.0001])[idx % 5]       # finite at every row with this noise
    sigmas = np.array([25.0, 1.0, 49.0])[idx % 3]
    seeds = list(range(100, 100 + A))
    gated = (idx % 4 != 2).astype(np.int32)
    spread = np.array([(0.0, 0.0, 0.0), (0.02, -0.01, 0.1), (-0.015, 0.02, -0.2), (0.01, 0.01, 0.3)])
    sims = np.stack([1.0 + 0.001 * idx, 1.0 - 0.0005 * idx, 10.0 + 0.01 * idx], axis=1)[:, None] + spread[None]
    sim_thr, real_thr = 0.04 + 0.001 * (idx % 30), 0.05 + 0.001 * (idx % 20)
    cost = MaxAbsThetaDot()
    batch = cacla.CACLA_SE_Batch(env, gammas, alphas, sigmas, seeds, None, sim_thr, real_thr, cost, gated=gated,
                                 sim_ensembles=sims)
    rewards, admitted = batch.run(steps)
    assert rewards.shape == (A, steps) and admitted.shape == (A, steps) and not batch.status.any()
    assert batch.worst_cost.shape == (A, steps) and batch.member_refusals.shape == (A, E)
    assert 0 < batch.admitted[gated != 0].sum() < steps * int(gated.sum())
    for a in range(A):
        if gated[a]:
            got, w, agent = single_ensemble(env, gammas[a], alphas[a], sigmas[a], seeds[a], steps, sims[a], cost,
                                            real_thr[a], sim_thr[a])
            assert np.array_equal(np.array(got), np.array(cacla.trim_rewards(rewards[a], admitted[a])))
            assert np.array_equal(agent.admitted_steps, admitted[a])
            assert (agent.admitted, agent.violations) == (batch.admitted[a], batch.violations[a])
            assert agent.first_refused == (None if batch.first_refused[a] < 0 else batch.first_refused[a])
            assert same_bits(agent.worst_cost, batch.worst_cost[a])
            assert np.array_equal(agent.member_refusals, batch.member_refusals[a])
        else:
            got, w, agent = single.single_plain(env, gammas[a], alphas[a], sigmas[a], seeds[a], steps)
            assert np.array_equal(got, rewards[a]) and admitted[a].all()
            assert np.isnan(batch.worst_cost[a]).all() and not batch.member_refusals[a].any()
        assert np.array_equal(batch.weights[a], w)
        assert batch.actor_updates[a] == agent.actor_updates
        assert np.array_equal(batch.state[a], np.array(env.get_state()))      # env is left at the run's last state


def test_the_ensemble_agent_leaves_the_streams_where_the_plain_agent_does():
    env, steps, seed = sw.SwimmerEnv(n=3), 70, 5
    rows = cases.members(3, 5, 0.1)[1]
    _, _, plain = single.single_plain(env, 0.9, 0.01, 25.0, seed, steps)
    after_plain = np.random.standard_normal(), torch.rand(1).numpy()
    got, _, safe = single_ensemble(env, 0.9, 0.01, 25.0, seed, steps, rows, MaxAbsThetaDot(), 0.075, 0.05)
    after_safe = np.random.standard_normal(), torch.rand(1).numpy()
    assert after_safe[0] == after_plain[0] and np.array_equal(after_safe[1], after_plain[1])
    assert np.array_equal(safe.initial_weights, plain.initial_weights)
    assert 0 < safe.admitted < steps and safe.first_refused is not None
    assert len(got) == steps - int(np.flatnonzero(safe.admitted_steps)[0])
    assert safe.worst_cost.shape == (steps,) and safe.member_refusals.shape == (5,)
    refused = steps - safe.admitted                       # a member's refusal is the ensemble's; one of them is behind each
    assert safe.member_refusals.max() <= refused <= safe.member_refusals.sum()
    assert np.array_equal(safe.worst_cost <= 0.05, safe.admitted_steps)


def test_safe_compare_ensemble_trains_three_agents_per_seed():
    env, steps, seeds = sw.SwimmerEnv(n=3), 80, [3, 4, 5]
    members = cases.members(3, 5, 0.1)[0]
    cost, real_thr, sim_thr = MaxAbsThetaDot(), 0.075, 0.05
    out = cacla.swimmer_experiment.safe_compare_ensemble(env, members, 0.9, 0.01, 25.0, seeds, cost, real_thr, steps,
                                                         sim_threshold=sim_thr)
    for who in ("plain", "single", "ensemble"):
        assert out["rewards_" + who].shape == (3, steps)
        for key in ("admitted_", "violations_", "first_refused_"):
            assert out[key + who].shape == (3,)
    assert out["member_refusals"].shape == (3, 5) and out["worst_margin"].shape == (3,)
    assert (out["admitted_plain"] == steps).all() and (out["first_refused_plain"] == -1).all()
    assert (out["admitted_single"] < steps).all() and (out["admitted_ensemble"] < steps).all()
    for i, seed in enumerate(seeds):
        rewards, _, _ = single.single_plain(env, 0.9, 0.01, 25.0, seed, steps)
        assert same_bits(out["rewards_plain"][i], rewards)
        got, _, agent = single.single_safe(env, 0.9, 0.01, 25.0, seed, steps, cases.CENTRE, cost, real_thr, sim_thr)
        assert same_bits(cacla.trim_rewards(out["rewards_single"][i], ~np.isnan(out["rewards_single"][i])), got)
        assert (agent.admitted, agent.violations) == (out["admitted_single"][i], out["violations_single"][i])
        assert agent.first_refused == (None if out["first_refused_single"][i] < 0 else out["first_refused_single"][i])
    both = (out["first_refused_single"] >= 0) & (out["first_refused_ensemble"] >= 0)
    assert both.any() and (out["first_refused_ensemble"][both] <= out["first_refused_single"][both]).all()
    assert (out["worst_margin"] >= 0).all()
    assert np.isfinite(out["worst_margin"][out["admitted_ensemble"] > 0]).all()
    # the default simulator threshold is the real threshold itself
    loose = cacla.swimmer_experiment.safe_compare_ensemble(env, members, 0.9, 0.01, 25.0, seeds[:1], cost, real_thr,
                                                           steps)
    tight = cacla.swimmer_experiment.safe_compare_ensemble(env, members, 0.9, 0.01, 25.0, seeds[:1], cost, real_thr,
                                                           steps, sim_threshold=real_thr)
    for key in loose:
        assert np.array_equal(loose[key], tight[key], equal_nan=True), key
