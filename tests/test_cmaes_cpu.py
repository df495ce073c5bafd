"""The built-in CMA-ES of the estimator (ars/cmaes.py) and the C-ABI boundary of the population residual kernel
(sw_step_residual_pop_f64), without a GPU."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import swimmer_amd as sw
from swimmer_amd.ars import cmaes
import oracle

HEADER = os.path.join(ROOT, "include", "swimmer_hip.h")


def sphere(X):
    return np.sum(X ** 2, axis=1)


def ellipsoid(X):
    return np.sum(X ** 2 * np.array([1.0, 1e3, 1e6]), axis=1)


def rosenbrock(X):
    return np.sum(100 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1)


def test_default_parameters_for_three_unknowns():
    es = cmaes.CMAES(np.zeros(3))
    N, lam, mu = 3, 7, 3
    assert (es.lam, es.mu) == (lam, mu)
    w = math.log(4.0) - np.log([1.0, 2.0, 3.0])
    assert np.allclose(es.weights, w / w.sum(), rtol=0, atol=1e-15)
    assert abs(es.weights.sum() - 1.0) < 1e-15 and np.all(es.weights > 0)
    mueff = 1.0 / np.sum((w / w.sum()) ** 2)
    assert es.mueff == pytest.approx(mueff, rel=1e-14)
    assert es.cs == pytest.approx((mueff + 2) / (N + mueff + 5), rel=1e-14)
    assert es.damps == pytest.approx(1 + 2 * max(0.0, math.sqrt((mueff - 1) / (N + 1)) - 1) + es.cs, rel=1e-14)
    assert es.cc == pytest.approx((4 + mueff / N) / (N + 4 + 2 * mueff / N), rel=1e-14)
    assert es.c1 == pytest.approx(2 / ((N + 1.3) ** 2 + mueff), rel=1e-14)
    assert es.cmu == pytest.approx(min(1 - es.c1, 2 * (mueff - 2 + 1 / mueff) / ((N + 2) ** 2 + mueff)), rel=1e-14)
    assert es.max_generations == int(100 + 150 * 36 / math.sqrt(7))
    assert es.hist_len == 10 + math.ceil(90 / 7)
    assert es.sigma == 1.0


@pytest.mark.parametrize("fun,x0,xopt", [(sphere, [0.5, -0.3, 0.8], [0, 0, 0]),
                                         (ellipsoid, [0.5, -0.3, 0.8], [0, 0, 0]),
                                         (rosenbrock, [0.0, 0.0, 0.0], [1, 1, 1])])
def test_converges(fun, x0, xopt):
    es = cmaes.minimize(fun, np.array(x0), seed=3)
    assert es.best_f <= 1e-8
    assert np.abs(es.best_x - np.array(xopt)).max() < 1e-3
    assert es.stop_reason in ("tolfun", "tolx")
    assert es.evaluations == es.generations * es.lam


def test_same_seed_same_bits_other_seed_other_path():
    a = cmaes.minimize(rosenbrock, np.zeros(3), seed=7)
    b = cmaes.minimize(rosenbrock, np.zeros(3), seed=7)
    c = cmaes.minimize(rosenbrock, np.zeros(3), seed=8)
    assert np.array_equal(a.best_x, b.best_x) and a.best_f == b.best_f and a.generations == b.generations
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.C, b.C)
    assert not np.array_equal(a.best_x, c.best_x)


def test_global_numpy_stream_is_untouched():
    np.random.seed(1234)
    before = np.random.get_state()
    cmaes.minimize(sphere, np.ones(3), seed=0)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_infinite_half_space_still_converges_inside():
    opt = np.array([0.3, 0.2, -0.1])

    def f(X):
        v = np.sum((X - opt) ** 2, axis=1)
        return np.where(X[:, 0] < 0.0, np.inf, v)     # +inf on the half-space x0 < 0

    es = cmaes.minimize(f, np.array([1.0, 1.0, 1.0]), seed=0)
    assert es.best_f <= 1e-8 and np.abs(es.best_x - opt).max() < 1e-3


def test_nan_ranks_last_and_ties_go_to_the_lower_index():
    es = cmaes.CMAES(np.zeros(3), seed=0)
    X = es.ask()
    f = np.array([np.nan, 1.0, np.inf, 1.0, 2.0, np.nan, 3.0])
    es.tell(X, f)
    assert es.best_f == 1.0 and np.array_equal(es.best_x, X[1])


def test_infeasible_candidates_are_redrawn_before_scoring():
    seen = []

    def f(X):
        seen.append(X.copy())
        return np.sum((X - 2.0) ** 2, axis=1)

    es = cmaes.minimize(f, np.array([0.5, 0.5, 0.5]), seed=1, feasible=lambda x: bool(np.all(x > 0)))
    assert all(np.all(X > 0) for X in seen)
    assert es.best_f <= 1e-8


def test_stop_reason_is_set_and_maxiter_holds():
    es = cmaes.minimize(rosenbrock, np.zeros(3), seed=0, max_generations=5)
    assert es.stop_reason == "maxiter" and es.generations == 5
    es = cmaes.minimize(sphere, np.ones(3), seed=0)
    assert es.stop_reason in ("tolfun", "tolx", "conditioncov")


def _store(name):
    """Stored transitions (states, actions = P s, next states) of the reference's rollouts the estimator reads: the
    next_rows.npz store with its subset, or the one rollout ARSAgent's computed branch draws from safe_agent_db.npz."""
    if name == "next_rows":
        g = np.load(os.path.join(GOLDEN, "next_rows.npz"))
        P, tr, subset = g["est_policies"], g["est_trajectories"], g["est_subset"]
        m_i, l_i, k, h = (float(v) for v in g["est_guess"])
    else:
        g = np.load(os.path.join(GOLDEN, "safe_agent_db.npz"))
        P, tr = g["policies"], g["trajectories"]
        np.random.seed(11)                       # the safe-agent cases' gseed; capacity = 1
        subset = np.random.randint(0, len(tr), 1)
        m_i, l_i, k, h = 1.0, 1.0, 10.0, 1e-3
    S = np.concatenate([tr[j][:-1] for j in subset])
    A = np.concatenate([tr[j][:-1] @ np.asarray(P[j]).T for j in subset])
    Nx = np.concatenate([tr[j][1:] for j in subset])
    return S, A, Nx, h, np.array([m_i, l_i, k])


def _native_on_oracle(name, seed):
    """estimate_real_env_param(method="native")'s search with the CPU oracle's physics: the default CMA-ES on I(x),
    then the least-squares refinement in (k l / m, m l^2, k / m)."""
    S, A, Nx, h, x0 = _store(name)

    def nxt(x):
        m_i, l_i, k = x
        return oracle.step_batch(oracle.OracleParams.make(3, l_i, m_i, k, h), S, A)[0]

    def fpop(X):
        return np.array([np.linalg.norm(nxt(x) - Nx, axis=1).sum() for x in X])

    def feasible(x):
        return x[0] > 0 and x[1] > 0 and np.all(np.isfinite(x))

    def res(u):
        return (nxt(cmaes.from_constants(u)) - Nx).ravel()

    def cost(u):
        r = res(u)
        return r @ r

    def normal(u):
        r0 = res(u)
        J = np.stack([(res(u + e) - res(u - e)) / (2 * e.max()) for e in np.diag(1e-6 * np.abs(u))], 1)
        return J.T @ J, J.T @ r0

    es = cmaes.minimize(fpop, x0, seed=seed, feasible=feasible)
    u = cmaes.refine_least_squares(cost, normal, cmaes.to_constants(*es.best_x), feasible=lambda v: bool(np.all(v > 0)))
    return es, cmaes.from_constants(u), fpop(np.array([cmaes.from_constants(u)]))[0]


@pytest.mark.parametrize("name", ["next_rows", "safe_agent_db"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_native_search_recovers_the_reference_parameters_on_the_oracle(name, seed):
    """The default search (lambda = 7, cma's stopping rules) and its refinement, with the C oracle's physics, on the
    reference's own rollouts: [m_i, l_i, k] = [1.2, 0.8, 10.2] to 1e-6 at seeds 0-4."""
    es, x, f = _native_on_oracle(name, seed)
    assert es.lam == 7 and es.stop_reason is not None
    assert np.abs(x - np.array([1.2, 0.8, 10.2])).max() <= 1e-6, (name, seed, es.best_x, x, es.stop_reason)
    assert f <= es.best_f


def test_constants_map_round_trips():
    x = np.array([1.2, 0.8, 10.2])
    u = cmaes.to_constants(*x)
    assert np.allclose(u, [10.2 * 0.8 / 1.2, 1.2 * 0.64, 10.2 / 1.2], rtol=1e-15)
    assert np.allclose(cmaes.from_constants(u), x, rtol=1e-14)


def test_refinement_never_makes_the_point_worse():
    calls = []

    def cost(u):
        calls.append(1)
        return float(np.sum((u - 3.0) ** 2))

    def normal(u):
        return 2 * np.eye(3), 2 * (u - 3.0)     # J = I scaled: Gauss-Newton solves it in one step
    u = cmaes.refine_least_squares(cost, normal, np.zeros(3))
    assert np.allclose(u, 3.0, atol=1e-12)
    u = cmaes.refine_least_squares(lambda v: 0.0 if np.all(v == 0) else 1.0, normal, np.zeros(3))
    assert np.array_equal(u, np.zeros(3))


def test_population_entry_point_is_declared_and_exported():
    src = open(HEADER).read()
    assert "int sw_step_residual_pop_f64(const sw_params *base, int64_t n_cand, const double *cand, int64_t n_env," in src
    assert "#define SW_STATUS_PARAM 8" in src
    assert "sw_step_residual_pop_f64" in sw._lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(sw._lib.library_path()), "sw_step_residual_pop_f64")
    assert sw._lib.load().sw_abi_version() == 3


def test_population_entry_point_validates_without_gpu():
    lib = sw._lib.load()
    fn = lib.sw_step_residual_pop_f64
    ok = sw.SwParams.make(3)
    dev = ctypes.c_void_p(8)          # never dereferenced: validation comes first
    args = lambda p, n_cand, n_env, cand=dev: (ctypes.byref(p), n_cand, cand, n_env, dev, dev, dev, dev, None, None,
                                               None)
    assert fn(None, 7, dev, 16, dev, dev, dev, dev, None, None, None) == 1
    assert fn(*args(ok, 7, 16, cand=None)) == 1
    assert fn(ctypes.byref(ok), 7, dev, 16, dev, None, dev, dev, None, None, None) == 1
    assert fn(*args(ok, 0, 16)) == 3
    assert fn(*args(ok, 7, -1)) == 3
    assert fn(*args(ok, 524281, 16)) == 3
    twin = sw.SwParams.make(3, flags=4)
    assert fn(*args(twin, 7, 16)) == 4
    assert fn(*args(sw.SwParams.make(9), 7, 16)) == 2
    assert fn(*args(ok, 7, 0)) == 0                     # nothing to do, nothing written


def test_estimator_method_is_checked():
    from swimmer_amd.ars.estimator import Estimator
    est = Estimator.__new__(Estimator)
    with pytest.raises(ValueError, match="method"):
        est.estimate_real_env_param(method="nelder-mead")
