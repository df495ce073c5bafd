"""sw_step_residual_pop_f64 (a whole CMA-ES generation of I(x) in one launch), Estimator.I_population and the
built-in search estimate_real_env_param(method="native"), on the GPU."""
import os
import warnings

import numpy as np
import pytest
import torch

import swimmer_amd as sw
from swimmer_amd import kernels
from swimmer_amd.ars.database import Database
from swimmer_amd.ars.estimator import Estimator
from conftest import GOLDEN
from test_safe_ars_agent_cpu import DB, _close, _fixture, _params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRUE_X = np.array([1.2, 0.8, 10.2])          # m_i, l_i, k of next_rows.npz's real world



def _transitions(n, T, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    d, m = 2 * n + 2, n - 1
    s = torch.empty((d, T), dtype=torch.float64, device=DEV)
    s[0:2].uniform_(-0.5, 0.5, generator=g)
    s[2::2].uniform_(-np.pi, np.pi, generator=g)
    s[3::2].uniform_(-2, 2, generator=g)
    a = torch.empty((m, T), dtype=torch.float64, device=DEV).uniform_(-5, 5, generator=g)
    nx = s + torch.empty_like(s).uniform_(-1e-3, 1e-3, generator=g)
    return s, a, nx


def _candidates(lam, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.5, 1.5, lam), rng.uniform(0.5, 1.5, lam), rng.uniform(5, 15, lam)], 1)


def _ordered_sum(row):
    """value's documented order: lane l adds row[l], row[l + 64], ... from 0.0, then the shuffle tree."""
    s = np.zeros(64)
    for c in range(0, row.size, 64):
        chunk = row[c:c + 64]
        s[:chunk.size] = s[:chunk.size] + chunk
    off = 32
    while off >= 1:
        s = s[:off] + s[off:2 * off]
        off //= 2
    return s[0]


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("T", [1, 255, 256, 257, 4097, 1 << 20])
def test_partials_are_bit_identical_to_the_single_candidate_kernel(n, T):
    s, a, nx = _transitions(n, T, seed=n * 7919 + T)
    h = 1e-3
    base = sw.SwParams.make(n, 1.0, 1.0, 10.0, h)
    for lam in (1, 7, 64):
        X = _candidates(lam, seed=lam + n)
        cand = torch.as_tensor(np.ascontiguousarray(X), device=DEV)
        value, partial, status = kernels.step_residual_population(base, cand, s, a, nx)
        value2, _, _ = kernels.step_residual_population(base, cand, s, a, nx)
        torch.cuda.synchronize()
        assert status.eq(0).all()
        for j in range(lam):
            ref = kernels.step_residual(sw.SwParams.make(n, X[j, 0], X[j, 1], X[j, 2], h), s, a, nx)
            assert torch.equal(partial[j], ref), (n, T, lam, j)
        P, v = partial.cpu().numpy(), value.cpu().numpy()
        for j in range(lam):
            assert v[j] == _ordered_sum(P[j]), (n, T, lam, j)
            assert v[j] == pytest.approx(P[j].sum(), rel=1e-12)
        assert torch.equal(value, value2)                       # bit-reproducible


def test_invalid_candidate_is_nan_and_flagged_and_its_neighbours_are_unchanged():
    n, T = 3, 5000
    s, a, nx = _transitions(n, T, seed=5)
    base = sw.SwParams.make(n)
    X = _candidates(9, seed=3)
    value, partial, status = kernels.step_residual_population(base, torch.as_tensor(X, device=DEV), s, a, nx)
    for bad in ([-1.0, 1.0, 10.0], [1.0, 0.0, 10.0], [1.0, 1.0, np.inf], [np.nan, 1.0, 10.0]):
        Y = X.copy()
        Y[4] = bad
        v, p, st = kernels.step_residual_population(base, torch.as_tensor(Y, device=DEV), s, a, nx)
        assert st.cpu().tolist() == [0] * 4 + [8] + [0] * 4
        assert torch.isnan(v[4]) and torch.isnan(p[4]).all()
        keep = [0, 1, 2, 3, 5, 6, 7, 8]
        assert torch.equal(v[keep], value[keep]) and torch.equal(p[keep], partial[keep])


def _next_rows_estimator():
    g = np.load(os.path.join(GOLDEN, "next_rows.npz"))
    H = g["est_trajectories"].shape[1]
    db = Database()
    for P, tr in zip(g["est_policies"], g["est_trajectories"]):
        db.add_trajectory(tr.tolist(), P)
    m_i, l_i, k, h = (float(v) for v in g["est_guess"])
    guess = sw.EnvParam("Simulator with estimation", n=3, H=H, l_i=l_i, m_i=m_i, h=h, k=k, epsilon=0.01)
    np.random.seed(12)
    est = Estimator(db, guess, capacity=len(g["est_subset"]))
    assert np.array_equal(est.subset, g["est_subset"])
    return est, g


def test_I_population_matches_the_reference_in_one_call():
    est, g = _next_rows_estimator()
    f = est.I_population(g["est_x"])
    assert f.shape == (3,)
    for got, want in zip(f, g["est_I"]):
        if want == 0.0:
            assert got < 1e-11
        else:
            assert got == pytest.approx(want, rel=1e-9)
    for x, got in zip(g["est_x"], f):                           # the same sums as I(x), another order
        assert got == pytest.approx(est.I(x), rel=1e-12, abs=1e-15)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_native_search_recovers_the_real_parameters(seed, monkeypatch):
    """The default search (lambda = 7, cma's stopping rules, then the least-squares refinement) on the reference's
    236-transition store: [1.2, 0.8, 10.2] to 1e-6, one population launch per generation, I(x) never called."""
    est, _ = _next_rows_estimator()
    launches = []
    inner = kernels.step_residual_population

    def counting(*a, **kw):
        launches.append(1)
        return inner(*a, **kw)

    def no_single(x):
        raise AssertionError("I(x) must not be called by the native search")

    monkeypatch.setattr(kernels, "step_residual_population", counting)
    monkeypatch.setattr(est, "I", no_single)
    ep = est.estimate_real_env_param(method="native", seed=seed)
    x = np.array([ep.m_i, ep.l_i, ep.k])
    assert np.abs(x - TRUE_X).max() <= 1e-6, (est.stop_reason, x)
    # one launch per generation, and one more that scores the refined point
    assert len(launches) == est.generations + 1 and est.evaluations == est.generations * 7
    assert est.stop_reason in ("tolfun", "tolx", "conditioncov", "maxiter")
    assert est.best_f < 1e-9


@pytest.mark.parametrize("tag", "hef")
def test_safe_agent_with_computed_estimation_matches_the_reference(tag, tmp_path, capsys):
    g = _fixture()
    ep, ap, thresh, c = _params(g, tag)
    w0 = str(tmp_path / f"w0_{tag}.npy")
    np.save(w0, g[tag + "_w0"])
    ap.initial_w = w0
    np.random.seed(c["gseed"])
    guess = sw.EnvParam("Simulator with estimation", n=3, H=20, l_i=1.0, m_i=1.0, k=10.0, h=1e-3, epsilon=0.0)
    agent = sw.ARSAgent(ep, ap, data_path=DB, seed=c["seed"], guess_param=guess, sim_thresh=thresh,
                        estimator_options={"method": "native"})
    assert "Using computed estimation..." in capsys.readouterr().out
    est = agent.estimated_param
    assert est.n == 3 and est.H == 20 and est.h == 1e-3
    assert np.abs(np.array([est.l_i, est.m_i, est.k]) - np.array([0.8, 1.2, 10.2])).max() <= 1e-6, est
    assert agent.sim_threshold == g[tag + "_sim_threshold"]
    per_it = []
    inner = agent.runOneIteration

    def recorded():
        r = inner()
        per_it.append(r)
        return r
    agent.runOneIteration = recorded
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        curve = agent.runTraining()
    counts = np.array([len(r) for r in per_it])
    assert np.array_equal(counts, g[tag + "_counts"])
    for j, r in enumerate(per_it):
        _close(r, g[tag + "_returns"][j][:len(r)])
    _close(curve, g[tag + "_curve"])
    _close(agent.policy, g[tag + "_policy"])
    assert agent.violations == int(g[tag + "_below"])
