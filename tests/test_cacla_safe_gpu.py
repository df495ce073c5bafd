"""CACLA behind the simulator gate (sw_cacla_safe_run_f64) on the GPU: parity with tests/cacla_safe_oracle.py at
every segment count where the kernel takes another shape, ungated agents against the plain kernel, batch rows against
the single classes, split runs, containment of a bad simulator and of a NaN threshold, and the random streams.

Bounds: 1e-9 absolute against the oracle on rewards, final weights and state -- the project's standing bound for runs
of this length (tests/test_cacla_gpu.py, tests/test_hip_parity.py); masks, counters and first refusals equal.  The
inputs are chosen so that every decision of a run (both thresholds, the sign of temp_diff) is at least 1e-6 from its
edge in the oracle's own run, which the tests assert before they compare: 1e-9 of rounding cannot flip one.  Ungated
agents, batch rows and split runs are compared bit for bit."""
import numpy as np
import pytest
import torch

import swimmer_amd as sw
from conftest import observed
from swimmer_amd import cacla
from swimmer_amd.cacla import safe_kernels
from swimmer_amd.safe_ars import AbsObs, MaxAbsThetaDot

import cacla_oracle
import cacla_safe_oracle as oracle_se

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIM = (1.02, 0.97, 10.3)          # the simulator of the parity cases; the real swimmer is (1, 1, 10)
STEPS = 96                        # crosses one 64-step block and ends in a partial one
GAMMA, ALPHA = 0.9, 0.01
# tag: n, cost, noise variance, sim_thresh, real_thresh.  Weights uniform +-0.3 from RandomState(1), noise from
# RandomState(1001): found with the oracle on the CPU; what each case contributes is asserted below.
CASES = {
    "n2": (2, "max", 25.0, 0.05, 0.075),
    "n3": (3, "max", 25.0, 0.05, 0.075),
    "n5": (5, "max", 25.0, 0.07, 0.105),
    "n6": (6, "max", 49.0, 0.10, 0.15),
    "n8": (8, "max", 25.0, 0.05, 0.04),     # real_thresh below sim_thresh: violations are counted
    "n3_abs3": (3, "abs3", 25.0, 0.05, 0.075),
}
_oracle, _seen = {}, {}


def costs(kind):
    return (MaxAbsThetaDot(), oracle_se.max_abs_thetadot) if kind == "max" else (AbsObs(3), oracle_se.abs_obs(3))


def inputs(tag):
    n, kind, var, sim_thr, real_thr = CASES[tag]
    w = np.random.RandomState(1).uniform(-0.3, 0.3, (n, cacla_oracle.net_doubles(n)))
    noise = np.random.RandomState(1001).normal(0.0, np.sqrt(var), (STEPS, n - 1))
    return n, kind, w, noise, sim_thr, real_thr


def want(tag):
    """The oracle's run of a case, computed once."""
    if tag not in _oracle:
        n, kind, w, noise, sim_thr, real_thr = inputs(tag)
        _oracle[tag] = oracle_se.run(n, GAMMA, ALPHA, w, noise, costs(kind)[1], SIM, sim_thr, real_thr)
    return _oracle[tag]


def t64(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=DEV)


def launch(n, cost, gamma, alpha, noise, gated, sim, sim_thr, real_thr, w0, parts=None, s0=None):
    """Runs of A agents through the wrapper, as one launch or split into `parts`.  -> dict of host arrays."""
    p = sw.SwParams.make(n)
    A, steps = noise.shape[0], noise.shape[1]
    w = t64(w0).clone()
    s = t64(np.tile(np.array(sw.SwimmerEnv(n=n).reset()), (A, 1)) if s0 is None else s0).clone()
    noise = t64(noise)
    last = torch.full((A,), float("nan"), dtype=torch.float64, device=DEV)
    counters = torch.zeros((A, 3), dtype=torch.int32, device=DEV)
    first = torch.full((A,), -1, dtype=torch.int32, device=DEV)
    status = torch.zeros(A, dtype=torch.int32, device=DEV)
    args = (t64(gamma), t64(alpha))
    gate = (torch.as_tensor(np.asarray(gated, dtype=np.int32), device=DEV), t64(sim), t64(sim_thr), t64(real_thr))
    rewards, rec, t = [], [], 0
    for c in (parts or [steps]):
        r = torch.empty((A, c), dtype=torch.int32, device=DEV)
        rewards.append(safe_kernels.cacla_safe_run(p, c, t, *args, noise[:, t:t + c].contiguous(), *gate, cost.kind,
                                                   cost.index, w, s, last, counters, first, admitted_rec=r,
                                                   status=status))
        rec.append(r)
        t += c
    return dict(rewards=torch.cat(rewards, dim=1).cpu().numpy(), admitted=torch.cat(rec, dim=1).cpu().numpy(),
                weights=w.cpu().numpy(), state=s.cpu().numpy(), last=last.cpu().numpy(),
                counters=counters.cpu().numpy(), first=first.cpu().numpy(), status=status.cpu().numpy())


# ---- (a) oracle parity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(CASES))
def test_a_gated_agent_against_the_oracle(tag):
    n, kind, w, noise, sim_thr, real_thr = inputs(tag)
    o = want(tag)
    adm = o["admitted"]
    assert adm.sum() >= 4 and (~adm).sum() >= 4, adm.sum()
    assert min(o["min_sim_margin"], o["min_real_margin"], o["min_td"]) >= 1e-6, o
    g = launch(n, costs(kind)[0], [GAMMA], [ALPHA], noise[None], [1], [SIM], [sim_thr], [real_thr], w[None])
    nan = np.isnan(o["rewards"])
    fig = {"rewards": float(np.abs(g["rewards"][0][~nan] - o["rewards"][~nan]).max()),
           "weights": float(np.abs(g["weights"][0] - o["weights"]).max()),
           "state": float(np.abs(g["state"][0] - o["state"]).max()),
           "admitted": int(adm.sum()), "counters": [int(v) for v in o["counters"]],
           "oracle_min_sim_margin": float(o["min_sim_margin"]), "oracle_min_real_margin": float(o["min_real_margin"]),
           "oracle_min_td": float(o["min_td"])}
    _seen[tag] = fig
    observed("cacla_safe_parity", _seen)
    assert np.array_equal(g["admitted"][0].astype(bool), adm)
    assert np.array_equal(np.isnan(g["rewards"][0]), nan)
    assert tuple(g["counters"][0]) == tuple(o["counters"])
    assert g["first"][0] == (-1 if o["first_refused"] is None else o["first_refused"])
    assert g["status"][0] == 0
    assert fig["rewards"] <= 1e-9 and fig["weights"] <= 1e-9 and fig["state"] <= 1e-9, fig


def test_the_parity_cases_cover_what_they_are_meant_to():
    """Over the cases: a refusal at step 0, an admitted step 0, a block boundary (steps 63 / 64) with a refusal on one
    side, actor updates, and counted violations with real_thresh below sim_thresh.  (The oracle alone.)"""
    runs = {tag: want(tag) for tag in CASES}
    assert any(not o["admitted"][0] and o["first_refused"] == 0 for o in runs.values())
    assert any(o["admitted"][0] for o in runs.values())
    assert any(o["admitted"][63] != o["admitted"][64] for o in runs.values())
    assert any(o["counters"][2] > 0 for o in runs.values())
    assert any(CASES[tag][4] < CASES[tag][3] and o["counters"][1] > 0 for tag, o in runs.items())
    assert runs["n6"]["counters"][2] > 0          # two hidden units per lane, with actor updates


# ---- the classes ---------------------------------------------------------------------------------------------------
def single_plain(env, gamma, alpha, sigma, seed, steps):
    torch.manual_seed(seed)
    np.random.seed(seed)
    agent = cacla.CACLA_agent(gamma, alpha, sigma)
    rewards = np.array(agent.run(env, steps))
    return rewards, np.concatenate([agent.actor_weights, agent.critic_weights[None]]), agent


def single_safe(env, gamma, alpha, sigma, seed, steps, sim, cost, real_thr, sim_thr):
    torch.manual_seed(seed)
    np.random.seed(seed)
    sim_env = sw.SwimmerEnv(n=env.n, l_i=sim[0], m_i=sim[1], k=sim[2])
    agent = cacla.CACLA_SE_agent(gamma, alpha, sigma, sim_env, cost, real_thr, sim_thr)
    rewards = agent.run(env, steps)
    return rewards, np.concatenate([agent.actor_weights, agent.critic_weights[None]]), agent


# ---- (b) ungated is the plain kernel -------------------------------------------------------------------------------
def same_bits(a, b):
    """Equal as 64-bit patterns: NaNs included (at n = 7 one ungated row overflows), and -0.0 is not 0.0."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("n", range(2, 9))        # every instantiation of both kernels
def test_ungated_rows_are_the_plain_kernel_bit_for_bit(n):
    env, steps, A = sw.SwimmerEnv(n=n), 100, 6
    gammas, alphas, sigmas = np.linspace(0.5, 0.95, A), [0.1, 0.01, 0.03] * 2, [1.0, 25.0, 0.1] * 2
    seeds, gated = list(range(40, 40 + A)), [0, 1, 0, 0, 1, 0]
    batch = cacla.CACLA_SE_Batch(env, gammas, alphas, sigmas, seeds, [SIM] * A, [0.05] * A, [0.04] * A,
                                 MaxAbsThetaDot(), gated=gated)
    rewards, admitted = batch.run(steps)
    plain = cacla.CACLABatch(env, gammas, alphas, sigmas, seeds)
    r_plain = plain.run(steps)
    free = [a for a in range(A) if not gated[a]]
    assert plain.actor_updates[free].sum() > 0 and not np.array_equal(plain.weights, batch.weights)
    assert same_bits(rewards[free], r_plain[free])
    assert same_bits(batch.weights[free], plain.weights[free])
    assert same_bits(batch.state[free], plain.state[free])
    assert np.array_equal(batch.actor_updates[free], plain.actor_updates[free])
    assert np.array_equal(batch.status[free], plain.status[free])
    assert admitted[free].all() and (batch.admitted[free] == steps).all() and (batch.first_refused[free] == -1).all()
    assert (batch.admitted[[1, 4]] < steps).all()         # the gated rows did meet their gate


# ---- (c) batch rows are single agents ------------------------------------------------------------------------------
def test_batch_rows_are_the_single_classes_bit_for_bit():
    env, steps, A = sw.SwimmerEnv(n=3), 100, 67
    idx = np.arange(A)
    gammas = np.linspace(0.1, 0.95, A)
    alphas = np.array([0.01, 0.003, 0.001, 0.0003, 0.0001])[idx % 5]       # finite at every row with this noise
    sigmas = np.array([25.0, 1.0, 49.0])[idx % 3]
    seeds = list(range(100, 100 + A))
    gated = (idx % 4 != 2).astype(np.int32)
    sims = np.stack([1.0 + 0.001 * idx, 1.0 - 0.0005 * idx, 10.0 + 0.01 * idx], axis=1)
    sim_thr, real_thr = 0.04 + 0.001 * (idx % 30), 0.05 + 0.001 * (idx % 20)
    cost = MaxAbsThetaDot()
    batch = cacla.CACLA_SE_Batch(env, gammas, alphas, sigmas, seeds, sims, sim_thr, real_thr, cost, gated=gated)
    rewards, admitted = batch.run(steps)
    assert rewards.shape == (A, steps) and admitted.shape == (A, steps) and not batch.status.any()
    assert 0 < batch.admitted[gated != 0].sum() < steps * int(gated.sum())
    for a in range(A):
        if gated[a]:
            got, w, agent = single_safe(env, gammas[a], alphas[a], sigmas[a], seeds[a], steps, sims[a], cost,
                                        real_thr[a], sim_thr[a])
            assert np.array_equal(np.array(got), np.array(cacla.trim_rewards(rewards[a], admitted[a])))
            assert np.array_equal(agent.admitted_steps, admitted[a])
            assert (agent.admitted, agent.violations) == (batch.admitted[a], batch.violations[a])
            assert agent.first_refused == (None if batch.first_refused[a] < 0 else batch.first_refused[a])
        else:
            got, w, agent = single_plain(env, gammas[a], alphas[a], sigmas[a], seeds[a], steps)
            assert np.array_equal(got, rewards[a]) and admitted[a].all()
        assert np.array_equal(batch.weights[a], w)
        assert batch.actor_updates[a] == agent.actor_updates
        assert np.array_equal(batch.state[a], np.array(env.get_state()))      # env is left at the run's last state


# ---- (d) splitting changes nothing -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (3, 6))
def test_splitting_a_run_changes_nothing(n):
    A, steps = 3, 150
    rs = np.random.RandomState(n)
    w0 = np.stack([cacla.draw_networks(n, torch.Generator().manual_seed(s)) for s in (1, 2, 3)])
    noise = rs.normal(0.0, [[[5.0]], [[7.0]], [[10.0]]], size=(A, steps, n - 1))
    args = (n, MaxAbsThetaDot(), [0.9, 0.5, 0.95], [0.01, 0.003, 0.003], noise, [1, 0, 1], [SIM] * A,
            [0.05, 0.05, 0.1], [0.04, 0.04, 0.08], w0)
    whole = launch(*args)
    assert not whole["status"].any() and whole["counters"][:, 2].sum() > 0
    assert 0 < whole["counters"][0, 0] < steps and 0 < whole["counters"][2, 0] < steps
    assert whole["counters"][1, 0] == steps and (whole["first"][[0, 2]] >= 0).all()
    for parts in ([64, 86], [1, 149]):
        split = launch(*args, parts=parts)
        for key in whole:
            assert np.array_equal(whole[key], split[key], equal_nan=True), (parts, key)


# ---- (e) containment -------------------------------------------------------------------------------------------------
def test_a_bad_simulator_and_a_nan_threshold_stay_contained():
    n, A, steps = 3, 4, 96
    rs = np.random.RandomState(11)
    w0 = rs.uniform(-0.3, 0.3, (A, n, cacla_oracle.net_doubles(n)))
    noise = rs.normal(0.0, 5.0, size=(A, steps, n - 1))
    sims = np.array([SIM, (-1.0, 0.97, 10.3), SIM, SIM])
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
    keep = [0, 3]
    alone = launch(n, cost, [0.9] * 2, [0.01] * 2, noise[keep], [1] * 2, sims[keep], sim_thr[keep], real_thr[keep],
                   w0[keep])
    assert 0 < alone["counters"][0, 0] < steps
    for key in g:
        assert np.array_equal(g[key][keep], alone[key], equal_nan=True), key


# ---- (f) drop-in streams ---------------------------------------------------------------------------------------------
def test_the_safe_agent_leaves_the_streams_where_the_plain_agent_does():
    env, steps, seed = sw.SwimmerEnv(n=3), 70, 5
    _, _, plain = single_plain(env, 0.9, 0.01, 25.0, seed, steps)
    after_plain = np.random.standard_normal(), torch.rand(1).numpy()
    got, _, safe = single_safe(env, 0.9, 0.01, 25.0, seed, steps, SIM, MaxAbsThetaDot(), 0.075, 0.05)
    after_safe = np.random.standard_normal(), torch.rand(1).numpy()
    assert after_safe[0] == after_plain[0] and np.array_equal(after_safe[1], after_plain[1])
    assert np.array_equal(safe.initial_weights, plain.initial_weights)
    assert 0 < safe.admitted < steps and safe.first_refused is not None
    assert len(got) == steps - int(np.flatnonzero(safe.admitted_steps)[0])


def test_safe_compare_pairs_a_plain_and_a_safe_agent_per_seed():
    env, sim = sw.SwimmerEnv(n=3), sw.SwimmerEnv(n=3, l_i=SIM[0], m_i=SIM[1], k=SIM[2])
    seeds, steps = [3, 4, 5], 80
    out = cacla.swimmer_experiment.safe_compare(env, sim, 0.9, 0.01, 25.0, seeds, MaxAbsThetaDot(), 0.075, 0.05, steps)
    assert out["rewards_plain"].shape == out["rewards_safe"].shape == (3, steps)
    assert (out["admitted_plain"] == steps).all() and (out["admitted_safe"] < steps).all()
    assert (out["first_refused"] >= 0).all()
    for i, seed in enumerate(seeds):
        rewards, _, _ = single_plain(env, 0.9, 0.01, 25.0, seed, steps)
        assert np.array_equal(out["rewards_plain"][i], rewards)
        # the pair parts only at the safe agent's first refusal
        k = out["first_refused"][i]
        assert np.array_equal(out["rewards_safe"][i][:k], rewards[:k])
    assert out["violations_plain"].shape == out["violations_safe"].shape == (3,)
