"""The lock-step drivers of the estimator batch (cmaes.minimize_many, cmaes.refine_least_squares_many), the C-ABI
boundary of its two kernels (sw_step_residual_sets_f64, sw_step_residual_normal_sets_f64) and EstimatorBatch's
construction, without a GPU."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import swimmer_amd as sw
from swimmer_amd.ars import cmaes
from swimmer_amd.ars.database import Database
from swimmer_amd.ars.estimator_batch import EstimatorBatch

HEADER = os.path.join(ROOT, "include", "swimmer_hip.h")


# ---- minimize_many ------------------------------------------------------------------------------------------------
def _quadratic(scales, opt):
    scales, opt = np.asarray(scales, dtype=np.float64), np.asarray(opt, dtype=np.float64)
    return lambda X: np.sum((X - opt) ** 2 * scales, axis=1)


def _rosenbrock(X):
    return np.sum(100 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1)


# six searches in N = 3: other conditioning, other optimum, one stopped at 5 generations, one behind a rule that
# refuses the half-space x0 <= 0
FUNS = [_quadratic([1, 1, 1], [0, 0, 0]), _quadratic([1, 1e3, 1e6], [0.3, -0.2, 0.1]), _rosenbrock,
        _quadratic([1, 10, 100], [2, 2, 2]), _rosenbrock, _quadratic([1e4, 1, 1e2], [-1, 0.5, 0.25])]
X0S = [[0.5, -0.3, 0.8], [0.5, -0.3, 0.8], [0, 0, 0], [0.5, 0.5, 0.5], [0.1, 0.2, 0.3], [1, 1, 1]]
SEEDS = [3, 1, 4, 1, 5, 9]
MAX_GEN = [None, None, None, None, 5, None]
FEASIBLE = [None, None, None, lambda x: bool(x[0] > 0), None, None]


def test_minimize_many_ends_every_instance_where_minimize_ends_it():
    calls = []

    def fun_many(idx, Xs):
        calls.append(list(idx))
        assert len(idx) == len(Xs)
        return [FUNS[i](X) for i, X in zip(idx, Xs)]

    many = cmaes.minimize_many(fun_many, X0S, seeds=SEEDS, feasibles=FEASIBLE, max_generations=MAX_GEN)
    assert len(many) == 6
    for i, es in enumerate(many):
        one = cmaes.minimize(FUNS[i], np.array(X0S[i], dtype=np.float64), seed=SEEDS[i], feasible=FEASIBLE[i],
                             max_generations=MAX_GEN[i])
        assert np.array_equal(es.best_x, one.best_x) and es.best_f == one.best_f, i
        assert (es.generations, es.evaluations, es.stop_reason) == (one.generations, one.evaluations, one.stop_reason)
        assert np.array_equal(es.mean, one.mean) and es.sigma == one.sigma and np.array_equal(es.C, one.C), i
    gens = [es.generations for es in many]
    assert many[4].stop_reason == "maxiter" and gens[4] == 5
    assert len(set(gens)) >= 2
    # one call per generation for everybody, never with a stopped instance
    assert len(calls) == max(gens)
    for g, idx in enumerate(calls):
        assert idx == [i for i in range(6) if gens[i] > g], g


def test_minimize_many_does_not_touch_the_global_numpy_stream():
    np.random.seed(99)
    before = np.random.get_state()
    cmaes.minimize_many(lambda idx, Xs: [FUNS[0](X) for X in Xs], X0S[:2], seeds=[0, 1], max_generations=3)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


# ---- refine_least_squares_many ------------------------------------------------------------------------------------
T_GRID = np.linspace(0.0, 2.0, 25)


def _expfit(true):
    """y = a exp(-b t) + c sampled on T_GRID: residuals and their exact Jacobian."""
    true = np.asarray(true, dtype=np.float64)
    y = true[0] * np.exp(-true[1] * T_GRID) + true[2]

    def res(u):
        return u[0] * np.exp(-u[1] * T_GRID) + u[2] - y

    def cost(u):
        r = res(u)
        return float(r @ r)

    def normal(u):
        e = np.exp(-u[1] * T_GRID)
        J = np.stack([e, -u[0] * T_GRID * e, np.ones_like(T_GRID)], 1)
        return J.T @ J, J.T @ res(u)
    return cost, normal


FITS = [_expfit(t) for t in ([2.0, 1.5, 0.5], [1.0, 0.7, 0.2], [3.0, 2.5, 1.0], [0.5, 0.3, 0.1])]
U0 = [np.array([1.0, 1.0, 0.0]), np.array([1.0, 0.7, 0.2]),      # the second one starts at its optimum
      np.array([2.0, 1.0, 0.5]), np.array([1.0, 1.0, 1.0])]
# the fourth one's rule refuses b < 0.6 while its optimum has b = 0.3: the first Gauss-Newton steps from b = 1 are
# blocked until the damping has shortened them
FIT_FEASIBLE = [None, None, None, lambda u: bool(u[1] >= 0.6)]


def test_refine_many_is_bit_equal_to_the_single_function():
    calls = {"cost": [], "normal": []}

    def cost_many(idx, U):
        calls["cost"].append(list(idx))
        return [FITS[i][0](u) for i, u in zip(idx, U)]

    def normal_many(idx, U):
        calls["normal"].append(list(idx))
        return [FITS[i][1](u) for i, u in zip(idx, U)]

    many = cmaes.refine_least_squares_many(cost_many, normal_many, U0, feasible=FIT_FEASIBLE)
    blocked = []
    for i in range(4):
        def feas(u, i=i):
            ok = FIT_FEASIBLE[i](u)
            if not ok:
                blocked.append(i)
            return ok
        one = cmaes.refine_least_squares(FITS[i][0], FITS[i][1], U0[i], feasible=feas if FIT_FEASIBLE[i] else None)
        assert np.array_equal(many[i], one), (i, many[i], one)
    assert np.array_equal(many[1], U0[1])                       # started at its optimum: stays
    assert np.abs(many[0] - [2.0, 1.5, 0.5]).max() < 1e-6 and np.abs(many[2] - [3.0, 2.5, 1.0]).max() < 1e-6
    assert 3 in blocked                                          # the rule did refuse steps
    # the first round asks every instance's cost at once; afterwards a call never holds an instance twice
    assert calls["cost"][0] == [0, 1, 2, 3] and calls["normal"][0] == [0, 1, 2, 3]
    assert all(len(set(c)) == len(c) for c in calls["cost"] + calls["normal"])


def test_refine_single_function_is_a_driver_over_the_same_steps():
    steps = cmaes._refine_steps(U0[0], None, 50)
    kind, u = next(steps)
    assert kind == "cost" and np.array_equal(u, U0[0])
    kind, u = steps.send(FITS[0][0](u))
    assert kind == "normal" and np.array_equal(u, U0[0])


# ---- the C ABI ----------------------------------------------------------------------------------------------------
def test_both_entry_points_are_declared_and_exported():
    src = open(HEADER).read()
    assert "int sw_step_residual_sets_f64(const sw_params *base, int64_t n_set, const int64_t *set_begin," in src
    assert "int sw_step_residual_normal_sets_f64(const sw_params *base, int64_t n_set, const int64_t *set_begin," in src
    lib = ctypes.CDLL(sw._lib.library_path())
    for name in ("sw_step_residual_sets_f64", "sw_step_residual_normal_sets_f64"):
        assert name in sw._lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "#define SW_ABI_VERSION 3" in src and sw._lib.load().sw_abi_version() == 3


def test_sets_entry_point_validates_before_any_device_work():
    fn = sw._lib.load().sw_step_residual_sets_f64
    ok, twin = sw.SwParams.make(3), sw.SwParams.make(3, flags=4)
    P = ctypes.c_void_p(8)               # non-NULL, never dereferenced: every call below fails a check

    def call(p=ok, n_set=2, set_begin=P, max_len=16, n_cand=7, cand=P, cand_set=P, n_env=32, state=P, action=P,
             next_ref=P, partial=P, value=P, status=P):
        return fn(ctypes.byref(p) if p is not None else None, n_set, set_begin, max_len, n_cand, cand, cand_set,
                  n_env, state, action, next_ref, partial, value, status, None)

    assert call(p=None) == 1
    for name in ("set_begin", "cand", "cand_set", "state", "action", "next_ref", "partial"):
        assert call(**{name: None}) == 1, name
    assert call(n_set=0) == 3 and call(n_cand=0) == 3 and call(max_len=0) == 3 and call(n_env=0) == 3
    assert call(n_cand=524281) == 3 and call(max_len=33) == 3     # more groups than grid rows; a set longer than all
    assert call(p=twin) == 4
    assert call(p=sw.SwParams.make(9)) == 2
    assert call(p=sw.SwParams.make(3, l_i=-1.0)) == 4


def test_normal_sets_entry_point_validates_before_any_device_work():
    fn = sw._lib.load().sw_step_residual_normal_sets_f64
    ok, twin = sw.SwParams.make(3), sw.SwParams.make(3, flags=4)
    P = ctypes.c_void_p(8)

    def call(p=ok, n_set=2, set_begin=P, max_len=16, n_point=7, points=P, inv_2e=P, active=None, n_env=32, state=P,
             action=P, next_ref=P, partial=P, out=P, status=None):
        return fn(ctypes.byref(p) if p is not None else None, n_set, set_begin, max_len, n_point, points, inv_2e,
                  active, n_env, state, action, next_ref, partial, out, status, None)

    assert call(p=None) == 1
    for name in ("set_begin", "points", "inv_2e", "state", "action", "next_ref", "partial", "out"):
        assert call(**{name: None}) == 1, name
    assert call(n_set=0) == 3 and call(max_len=0) == 3 and call(n_env=0) == 3
    assert call(n_set=65536) == 3 and call(max_len=33) == 3
    for n_point in (0, 2, 6, 8, -1):
        assert call(n_point=n_point) == 4, n_point
    assert call(p=twin) == 4 and call(p=twin, n_point=1, inv_2e=None) == 4
    assert call(p=sw.SwParams.make(9)) == 2


# ---- EstimatorBatch's construction --------------------------------------------------------------------------------
def _next_rows():
    g = np.load(os.path.join(GOLDEN, "next_rows.npz"))
    db = Database()
    for P, tr in zip(g["est_policies"], g["est_trajectories"]):
        db.add_trajectory(tr.tolist(), P)
    m_i, l_i, k, h = (float(v) for v in g["est_guess"])
    guess = sw.EnvParam("Simulator with estimation", n=3, H=g["est_trajectories"].shape[1], l_i=l_i, m_i=m_i, h=h, k=k,
                        epsilon=0.01)
    return db, guess, g


def test_subsets_are_the_single_estimators_and_the_global_stream_is_untouched():
    db, guess, g = _next_rows()
    np.random.seed(4321)
    before = np.random.get_state()
    batch = EstimatorBatch(db, guess, capacity=4, seeds=[12])
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert batch.n_estimators == 1 and np.array_equal(batch.subsets[0], g["est_subset"])
    assert sw.EstimatorBatch is EstimatorBatch


def test_equal_subsets_on_one_store_share_a_set():
    db, guess, g = _next_rows()
    other = Database()
    for P, tr in zip(g["est_policies"], g["est_trajectories"]):
        other.add_trajectory(tr.tolist(), P)
    batch = EstimatorBatch(db, guess, capacity=4, seeds=[12, 3, 12, 12])
    assert batch.set_of == [0, 1, 0, 0] and batch.n_sets == 2
    batch = EstimatorBatch([db, other, db], guess, capacity=4, subsets=[[0, 1], [0, 1], [0, 1]])
    assert batch.set_of == [0, 1, 0] and batch.n_sets == 2        # the same indices into ANOTHER store: another set
    assert batch.seeds is None


def test_bad_arguments_raise():
    db, guess, _ = _next_rows()
    import dataclasses
    with pytest.raises(AssertionError, match="not the same"):
        EstimatorBatch(db, dataclasses.replace(guess, H=guess.H + 1), capacity=4, seeds=[0])
    with pytest.raises(AssertionError, match="empty"):
        EstimatorBatch(Database(), guess, capacity=4, seeds=[0])
    with pytest.raises(ValueError, match="share n and h"):
        EstimatorBatch(db, [guess, dataclasses.replace(guess, h=2e-3)], capacity=4, seeds=[0, 1])
    with pytest.raises(ValueError, match="seeds"):
        EstimatorBatch(db, guess, capacity=4)
    with pytest.raises(ValueError, match="subsets"):
        EstimatorBatch(db, guess, capacity=4, subsets=[[0, 99]])
    with pytest.raises(ValueError, match="native"):
        EstimatorBatch(db, guess, capacity=4, seeds=[0]).estimate(method="cma")
