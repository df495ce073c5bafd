"""CACLA on the fused kernel (sw_cacla_run_f64) on the GPU: drop-in parity with the reference's own runs
(tests/golden/cacla.npz), the segment counts without a golden against tests/cacla_oracle.py, batches, split runs and a
diverging agent.

Bounds: 1e-9 absolute against the reference's goldens and the oracle -- the project's standing bound for rollouts of
H <= 1000 steps (tests/test_hip_parity.py); the random-stream witnesses, batch rows and split runs are compared
exactly."""
import os

import numpy as np
import pytest
import torch

import swimmer_amd as sw
from conftest import GOLDEN, observed
from swimmer_amd import cacla

import cacla_oracle

pytestmark = pytest.mark.gpu

TRAIN_CASES = ("A", "B", "C", "D", "E")
_seen = {}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "cacla.npz"), allow_pickle=False)


def run_case(gold, tag):
    seed, n, gamma, alpha, sigma, steps, train = gold[f"{tag}_hyper"]
    torch.manual_seed(int(seed))
    np.random.seed(int(seed))
    agent = cacla.CACLA_agent(gamma, alpha, sigma)
    env = sw.SwimmerEnv(n=int(n))
    rewards = agent.run(env, int(steps), train=bool(train))
    assert isinstance(rewards, list) and len(rewards) == int(steps)
    w = np.concatenate([agent.actor_weights, agent.critic_weights[None]])
    figures = {"rewards": float(np.abs(np.array(rewards) - gold[f"{tag}_rewards"]).max()),
               "weights": float(np.abs(w - gold[f"{tag}_w1"]).max()),
               "state": float(np.abs(np.array(env.get_state()) - gold[f"{tag}_state"]).max())}
    _seen[tag] = figures
    observed("cacla_parity", _seen)
    assert np.array_equal(agent.initial_weights, gold[f"{tag}_w0"])
    assert agent.status == 0
    # the run consumed both global streams exactly as the reference's did
    assert np.random.standard_normal() == gold[f"{tag}_next_normal"]
    assert np.array_equal(torch.rand(1).numpy(), gold[f"{tag}_next_rand"])
    return agent, figures


@pytest.mark.parametrize("tag", TRAIN_CASES)
def test_drop_in_against_the_reference(gold, tag):
    _, fig = run_case(gold, tag)
    assert fig["rewards"] <= 1e-9 and fig["weights"] <= 1e-9 and fig["state"] <= 1e-9, fig


def test_train_false_is_the_reference_as_written(gold):
    """cacla_agent.py:173-178: no updates, the actors keep seeing the reset observation while the swimmer moves on
    (a kernel that advances `state` fails here)."""
    agent, fig = run_case(gold, "A0")
    assert fig["rewards"] <= 1e-9 and fig["state"] <= 1e-9, fig
    assert np.array_equal(np.concatenate([agent.actor_weights, agent.critic_weights[None]]), gold["A0_w0"])
    assert agent.actor_updates == 0


@pytest.mark.parametrize("n", (4, 6, 7))
def test_segment_counts_without_a_golden_against_the_oracle(n):
    """n = 6 is where two hidden units share a lane; 64 steps, every step compared."""
    seed, gamma, alpha, sigma, steps = 10 + n, 0.9, 0.01, 0.1, 64
    torch.manual_seed(seed)
    np.random.seed(seed)
    agent = cacla.CACLA_agent(gamma, alpha, sigma)
    env = sw.SwimmerEnv(n=n)
    rewards = np.array(agent.run(env, steps))
    noise = np.random.RandomState(seed).multivariate_normal(np.zeros(n - 1), sigma * np.identity(n - 1), size=steps)
    want = cacla_oracle.run(n, gamma, alpha, agent.initial_weights, noise)
    w = np.concatenate([agent.actor_weights, agent.critic_weights[None]])
    fig = {"rewards": float(np.abs(rewards - want["rewards"]).max()), "weights": float(np.abs(w - want["weights"]).max()),
           "state": float(np.abs(np.array(env.get_state()) - want["state"]).max()),
           "oracle_min_td": float(want["min_td"]), "oracle_min_z": float(want["min_z"])}
    _seen[f"oracle_n{n}"] = fig
    observed("cacla_parity", _seen)
    assert fig["rewards"] <= 1e-9 and fig["weights"] <= 1e-9 and fig["state"] <= 1e-9, fig
    assert agent.actor_updates == want["actor_updates"]


def single(env, gamma, alpha, sigma, seed, steps):
    torch.manual_seed(seed)
    np.random.seed(seed)
    agent = cacla.CACLA_agent(gamma, alpha, sigma)
    rewards = np.array(agent.run(env, steps))
    return rewards, np.concatenate([agent.actor_weights, agent.critic_weights[None]]), agent


def test_batch_rows_are_independent_agents_bit_for_bit():
    env, steps = sw.SwimmerEnv(n=3), 100
    A = 67
    gammas = np.linspace(0.1, 0.95, A)
    alphas = np.array([0.1, 0.03, 0.01, 0.003, 0.001])[np.arange(A) % 5]
    sigmas = np.array([1.0, 0.1, 0.001])[np.arange(A) % 3]
    seeds = list(range(100, 100 + A))
    small = cacla.CACLABatch(env, gammas[:3], alphas[:3], sigmas[:3], seeds[:3])
    r3 = small.run(steps)
    big = cacla.CACLABatch(env, gammas, alphas, sigmas, seeds)
    r67 = big.run(steps)
    assert r3.shape == (3, steps) and r67.shape == (A, steps) and big.weights.shape == (A, 3, cacla.net_doubles(3))
    assert not big.status.any()
    for a in (0, 1, 66):
        rewards, w, agent = single(env, gammas[a], alphas[a], sigmas[a], seeds[a], steps)
        assert np.array_equal(r67[a], rewards) and np.array_equal(big.weights[a], w)
        assert big.actor_updates[a] == agent.actor_updates
        if a < 3:
            assert np.array_equal(r3[a], rewards) and np.array_equal(small.weights[a], w)
    assert np.array_equal(r3, r67[:3])


@pytest.mark.parametrize("n", (3, 6))
def test_splitting_a_run_changes_nothing(n):
    """100 steps in one launch, as 37 + 63 and as 64 + 36: the reward staging's partial flush and the noise
    look-ahead at lengths that are no multiple of the 64-step block."""
    p, A, steps, dev = sw.SwParams.make(n), 3, 100, "cuda:0"
    rs = np.random.RandomState(n)
    w0 = np.stack([cacla.draw_networks(n, torch.Generator().manual_seed(s)) for s in (1, 2, 3)])
    noise = torch.as_tensor(rs.normal(0.0, [[[0.3]], [[1.0]], [[0.03]]], size=(A, steps, n - 1)), device=dev)
    gamma = torch.tensor([0.9, 0.5, 0.95], dtype=torch.float64, device=dev)
    alpha = torch.tensor([0.01, 0.1, 0.003], dtype=torch.float64, device=dev)
    s0 = np.tile(np.array(sw.SwimmerEnv(n=n).reset()), (A, 1))

    def go(parts):
        w, s = torch.as_tensor(w0, device=dev).clone(), torch.as_tensor(s0, device=dev).clone()
        upd = torch.zeros(A, dtype=torch.int32, device=dev)
        st = torch.zeros(A, dtype=torch.int32, device=dev)
        out, t = [], 0
        for c in parts:
            out.append(sw.kernels.cacla_run(p, c, True, gamma, alpha, noise[:, t:t + c].contiguous(), w, s,
                                            actor_updates=upd, status=st))
            t += c
        return torch.cat(out, dim=1).cpu().numpy(), w.cpu().numpy(), s.cpu().numpy(), upd.cpu().numpy(), st.cpu().numpy()
    whole = go([100])
    assert not whole[4].any() and np.isfinite(whole[0]).all() and whole[3].sum() > 0
    assert not np.array_equal(whole[1], w0)
    for parts in ([37, 63], [64, 36]):
        for a, b in zip(whole, go(parts)):
            assert np.array_equal(a, b), parts


def test_a_diverging_agent_stays_contained():
    """alpha = 1e6 overflows one agent's weights (floating point only); its neighbours do not notice."""
    env, steps, seeds = sw.SwimmerEnv(n=3), 256, [7, 8, 9]
    gammas, sigmas = [0.9, 0.9, 0.5], [0.1, 0.1, 1.0]
    with_it = cacla.CACLABatch(env, gammas, [0.01, 1e6, 0.1], sigmas, seeds)
    r = with_it.run(steps)
    without = cacla.CACLABatch(env, gammas[::2], [0.01, 0.1], sigmas[::2], seeds[::2])
    r2 = without.run(steps)
    assert with_it.status[1] & sw._lib.STATUS_NONFINITE
    bad = np.flatnonzero(~np.isfinite(r[1]))
    assert bad.size and np.isnan(r[1][bad[0]:]).all(), (bad[:4], r[1][bad[0]:bad[0] + 4])
    assert with_it.status[0] == 0 and with_it.status[2] == 0
    assert np.array_equal(r[[0, 2]], r2) and np.array_equal(with_it.weights[[0, 2]], without.weights)
    assert np.isfinite(r2).all()
