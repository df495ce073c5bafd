"""The RL-Glue ARS experiment on the GPU (sw_rlglue_ars_run_f64 behind swimmer_amd.rlglue): every golden case of the
reference's own agent within 10 x the reference's own recorded sensitivity, n = 7 against the NumPy restatement under
the same rule, the clip, batch against single and split against whole bit for bit, guards around every output, and a
diverging agent among healthy ones.  Every case is a few thousand environment steps at most (the shipped
parameters.txt: 9000)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rlglue_oracle  # noqa: E402
import swimmer_amd as sw  # noqa: E402
from swimmer_amd import rlglue  # noqa: E402
from conftest import observed  # noqa: E402
from test_rlglue_experiment_cpu import TAGS, case_of  # noqa: E402

pytestmark = pytest.mark.gpu
NONFINITE = sw._lib.STATUS_NONFINITE
FACTOR = 10.0          # x the recorded sensitivity: covers the small sample of perturbed runs behind it


def params_of(c, **over):
    kw = dict(n_seg=c["n"], direction=c["direction"], h_global=c["h"], N=c["N"], b=c["b"], H=c["H"], alpha=c["alpha"],
              nu=c["nu"], max_u=c["max_u"], l_i=c["l_i"], k=c["k"], m_i=c["m_i"])
    kw.update(over)
    return rlglue.Parameters(**kw)


def run_per_iteration(params, seed, iterations):
    """One agent, an iteration per call (so the policy after every update can be read): eval [it], rew [it, 2N],
    policies [it, m, d], status."""
    ex = rlglue.SwimmerExperimentBatch(params, [seed])
    policies = []
    for _ in range(iterations):
        ex.run(1)
        policies.append(ex.policy[0])
    return dict(eval=ex.eval_returns[0], rew=ex.train_returns[0], policies=np.array(policies),
                status=int(ex.status[0]))


def ratios(got, ref, sens):
    """max |got - ref| / sensitivity per quantity; 0 / 0 counts as 0 (an identically zero quantity reproduced)."""
    out = {}
    for key in ("eval", "rew", "policies"):
        err = float(np.abs(got[key] - ref[key]).max())
        out[key] = 0.0 if err == 0.0 else (err / sens[key] if sens[key] > 0 else float("inf"))
    return out


@pytest.fixture(scope="module")
def golden_runs(golden):
    g = golden.rlglue_ars
    runs = {}
    for tag in TAGS:
        c = case_of(g, tag)
        runs[tag] = run_per_iteration(params_of(c), c["seed"], c["iterations"])
    return runs


@pytest.fixture(scope="module")
def golden_ratios(golden, golden_runs):
    g = golden.rlglue_ars
    out = {}
    for tag in TAGS:
        if tag == "G":          # no finite policy to compare: test_h1_case
            continue
        ref = {k: g[f"{tag}_{k}"] for k in ("eval", "rew", "policies")}
        sens = {k: float(g[f"{tag}_sens_{k}"]) for k in ("eval", "rew", "policies")}
        out[tag] = ratios(golden_runs[tag], ref, sens)
    observed("rlglue_matrix_observed", {"error / recorded sensitivity (bound %g)" % FACTOR: out})
    return out


@pytest.mark.parametrize("tag", [t for t in TAGS if t != "G"])
def test_golden_case_within_the_references_sensitivity(golden_runs, golden_ratios, tag):
    print(tag, golden_ratios[tag])
    assert golden_runs[tag]["status"] == 0
    for key, ratio in golden_ratios[tag].items():
        assert ratio <= FACTOR, (tag, key, ratio)


def test_h1_case(golden, golden_runs):
    """H = 1: the reference's returns are all one number, its first update is 0 / 0 and its policy all NaN."""
    g, got = golden.rlglue_ars, golden_runs["G"]
    err = float(np.abs(got["rew"] - g["G_rew"]).max())
    print("G rew error / sensitivity", err / float(g["G_sens_rew"]))
    assert err <= FACTOR * float(g["G_sens_rew"])
    assert (got["rew"] == got["rew"][0, 0]).all()
    assert np.isnan(got["policies"]).all() and np.isnan(g["G_policies"]).all()
    assert np.array_equal(got["eval"], g["G_eval"]) and got["eval"][0] == 0.0
    assert got["status"] & NONFINITE
    c = case_of(g, "G")
    with pytest.raises(ValueError):
        rlglue.SwimmerExperiment(params_of(c), seed=c["seed"]).run(1)


def test_n7_against_the_restatement():
    n, N, b, H, alpha, nu, max_u, it, seed = 7, 2, 2, 12, 0.02, 0.05, 5.0, 4, 21
    deltas = np.random.RandomState(seed).rand(it + 1, N, n - 1, 2 * n + 2)

    def make(perturb=None):
        return rlglue_oracle.Run(n, N, b, H, alpha, nu, max_u, deltas, perturb=perturb)
    ref = make().run(it).arrays()
    sens = rlglue_oracle.sensitivity(make, it, ref)
    assert min(sens.values()) > 0 and sens["policies"] <= 1e-7
    got = run_per_iteration(rlglue.Parameters(n_seg=n, N=N, b=b, H=H, alpha=alpha, nu=nu, max_u=max_u), seed, it)
    r = ratios(got, ref, sens)
    observed("rlglue_n7_observed", {"sensitivity": sens, "error / sensitivity": r})
    assert got["status"] == 0
    assert max(r.values()) <= FACTOR, r


def test_clip_changes_the_run(golden, golden_runs):
    g = golden.rlglue_ars
    for tag in ("CLIP1", "CLIP2"):
        c = case_of(g, tag)
        free = run_per_iteration(params_of(c, max_u=float("inf")), c["seed"], c["iterations"])
        assert free["status"] == 0
        for key in ("eval", "rew", "policies"):
            assert not np.array_equal(free[key], golden_runs[tag][key]), (tag, key)
        wide = run_per_iteration(params_of(c, max_u=1e9), c["seed"], c["iterations"])     # a bound nothing reaches
        for key in ("eval", "rew", "policies"):
            assert np.array_equal(free[key], wide[key]), (tag, key)


BATCH = dict(n_seg=3, N=2, b=2, H=10, max_u=2e-3)
BATCH_IT = 3


def agent_settings(a):
    return 100 + 7 * a, 0.01 + 0.003 * (a % 5), 0.05 + 0.1 * (a % 3)      # seed, alpha, nu


@pytest.fixture(scope="module")
def singles():
    out = []
    for a in range(130):
        seed, alpha, nu = agent_settings(a)
        ex = rlglue.SwimmerExperiment(rlglue.Parameters(alpha=alpha, nu=nu, **BATCH), seed=seed)
        ev = ex.run(BATCH_IT)
        out.append((ev, ex.train_returns, ex.policy, ex.status))
    return out


@pytest.mark.parametrize("n_agent", [1, 2, 63, 64, 65, 130])
def test_batch_rows_are_the_single_experiments(singles, n_agent):
    sets = [agent_settings(a) for a in range(n_agent)]
    ex = rlglue.SwimmerExperimentBatch(rlglue.Parameters(**BATCH), [s[0] for s in sets], [s[1] for s in sets],
                                       [s[2] for s in sets])
    ev = ex.run(BATCH_IT)
    assert ev.shape == (n_agent, BATCH_IT) and ex.train_returns.shape == (n_agent, BATCH_IT, 4)
    assert ex.policy.shape == (n_agent, 2, 8)
    assert n_agent == 1 or not np.array_equal(ev[0], ev[-1])              # mixed settings: the rows differ
    for a in range(n_agent):
        s_ev, s_tr, s_pol, s_st = singles[a]
        assert np.array_equal(ev[a], s_ev) and np.array_equal(ex.train_returns[a], s_tr), a
        assert np.array_equal(ex.policy[a], s_pol) and ex.status[a] == s_st == 0, a


def test_split_runs_change_no_bit(monkeypatch):
    params = rlglue.Parameters(n_seg=4, N=2, b=1, H=15, alpha=0.03, nu=0.2, max_u=1e-3)
    seeds, alphas = [3, 4, 5], [0.03, 0.02, 0.05]
    whole = rlglue.SwimmerExperimentBatch(params, seeds, alphas)
    ev = whole.run(7)
    split = rlglue.SwimmerExperimentBatch(params, seeds, alphas)
    first, second = split.run(3), split.run(4)
    assert np.array_equal(np.concatenate([first, second], axis=1), ev)
    monkeypatch.setattr(rlglue.experiment, "CHUNK_ENV_STEPS", 2 * 5 * 15)                 # two iterations per launch
    chunked = rlglue.SwimmerExperimentBatch(params, seeds, alphas)
    assert chunked._chunk_iterations() == 2
    assert np.array_equal(chunked.run(7), ev)
    for other in (split, chunked):
        assert np.array_equal(other.policy, whole.policy) and np.array_equal(other.train_returns, whole.train_returns)
        assert np.array_equal(other.eval_returns, ev) and np.array_equal(other.status, whole.status)
        assert other._rng[0].rand() == np.random.RandomState(3).rand(8 * 2 * 3 * 10 + 1)[-1]
    single = rlglue.SwimmerExperiment(params, seed=3)
    assert np.array_equal(np.concatenate([single.run(3), single.run(4)]), ev[0]) and single.iterations == 7


def test_results_file(tmp_path):
    ex = rlglue.SwimmerExperiment(rlglue.Parameters(H=20, N=1), seed=1)
    ev = ex.run(3)
    path = tmp_path / "results.txt"
    ex.write_results(path)
    lines = path.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == 4
    for i, line in enumerate(lines[:3]):
        head, value = line.split(":")
        assert head == f"Reward for one rollout with policy at iteration {i}"
        assert abs(float(value) - ev[i]) <= 5e-6 * abs(ev[i])                             # six significant digits


def test_guards_around_every_output():
    n, N, b, H, it, A, G = 5, 2, 2, 6, 2, 65, 97
    p = sw.SwParams.make(n, h=0.01, flags=sw._lib.FLAG_MODEL_TWIN)
    m, d = p.m, p.d
    dev = torch.device("cuda:0")

    def guarded(shape, dtype=torch.float64, fill=float("nan"), inner=None):
        size = int(np.prod(shape))
        flat = torch.full((size + 2 * G,), fill, dtype=dtype, device=dev)
        view = flat[G:G + size].view(shape)
        if inner is not None:
            view.fill_(inner)
        return flat, view
    f_pol, policy = guarded((m, d, A), inner=0.0)
    f_car, carry = guarded((m + 1, A))                     # iter_begin = 0: never read, NaN on input
    f_ev, ev = guarded((it, A))
    f_tr, tr = guarded((it, 2 * N, A))
    f_st, status = guarded((A,), torch.int32, -7, inner=0)
    rs = np.random.RandomState(0)
    deltas = torch.as_tensor(rs.rand(it, N, m, d, A), device=dev)
    alpha = torch.full((A,), 0.02, dtype=torch.float64, device=dev)
    nu = torch.full((A,), 0.05, dtype=torch.float64, device=dev)
    sw.kernels.rlglue_ars_run(p, 5.0, 0, it, N, b, H, alpha, nu, deltas, policy, carry, status, ev, tr)
    torch.cuda.synchronize()
    for flat in (f_pol, f_car, f_ev, f_tr):
        assert torch.isnan(flat[:G]).all() and torch.isnan(flat[-G:]).all()
    assert (f_st[:G] == -7).all() and (f_st[-G:] == -7).all() and (status == 0).all()
    for view in (policy, carry, ev, tr):
        assert torch.isfinite(view).all()
    assert (policy != 0).all()
    # the same agents in a second call that continues from the carry: only its own entries move
    keep = [t.clone() for t in (f_pol, f_car)]
    sw.kernels.rlglue_ars_run(p, 5.0, it, it, N, b, H, alpha, nu, deltas, policy, carry, status, ev, tr)
    torch.cuda.synchronize()
    for flat, old in zip((f_pol, f_car), keep):
        assert torch.isnan(flat[:G]).all() and torch.isnan(flat[-G:]).all()
        assert not torch.equal(flat[G:-G], old[G:-G])


def test_a_diverging_agent_leaves_its_neighbours_alone():
    base = dict(n_seg=3, N=2, b=2, H=40, max_u=2e-3)
    it = 8
    seeds = [11, 12, 3, 13, 14]
    alphas, nus = [0.02, 0.03, 0.5, 0.02, 0.04], [0.05, 0.1, 1.0, 0.05, 0.2]
    ex = rlglue.SwimmerExperimentBatch(rlglue.Parameters(**base), seeds, alphas, nus)
    ev = ex.run(it)                                        # never raises
    assert ex.status[2] & NONFINITE and not np.isfinite(ev[2]).all()
    for a in (0, 1, 3, 4):
        alone = rlglue.SwimmerExperiment(rlglue.Parameters(alpha=alphas[a], nu=nus[a], **base), seed=seeds[a])
        assert np.array_equal(alone.run(it), ev[a]) and alone.status == 0 == ex.status[a]
        assert np.array_equal(alone.policy, ex.policy[a]) and np.array_equal(alone.train_returns, ex.train_returns[a])
    with pytest.raises(ValueError):
        rlglue.SwimmerExperiment(rlglue.Parameters(alpha=0.5, nu=1.0, **base), seed=3).run(it)
