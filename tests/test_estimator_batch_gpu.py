"""sw_step_residual_sets_f64 and sw_step_residual_normal_sets_f64 (the estimator batch's two kernels), EstimatorBatch
and the computed-simulator sweep of ars/safe_exploration.py, on the GPU."""
import os

import numpy as np
import pytest
import torch

import swimmer_amd as sw
from swimmer_amd import kernels
from swimmer_amd.ars import cmaes, safe_exploration
from swimmer_amd.ars.database import Database
from swimmer_amd.ars.estimator import Estimator
from swimmer_amd.ars.estimator_batch import EstimatorBatch
from conftest import GOLDEN
from test_estimator_population_gpu import _candidates, _ordered_sum, _transitions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRUE_X = np.array([1.2, 0.8, 10.2])          # m_i, l_i, k of both stores' real world
H_STEP = 1e-3


def _sets(n, lengths, seed):
    """Sets of synthetic transitions side by side -> (state, action, next_ref, set_begin on the device, begin)."""
    parts = [_transitions(n, T, seed=seed + 31 * i) for i, T in enumerate(lengths)]
    begin = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    s, a, nx = (torch.cat([p[j] for p in parts], 1).contiguous() for j in range(3))
    return s, a, nx, torch.as_tensor(begin, device=DEV), begin


# ---- kernel 1 -----------------------------------------------------------------------------------------------------
LENGTHS = [1, 255, 256, 257, 4097]
PER_SET = [1, 7, 0, 9, 8]        # a set without candidates; set 3's candidates straddle a group of 8 (8..16)
SENTINEL = -12345.0


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
def test_set_partials_are_bit_identical_to_the_single_candidate_kernel_on_each_slice(n):
    s, a, nx, set_begin, begin = _sets(n, LENGTHS, seed=n * 7919)
    base = sw.SwParams.make(n, 1.0, 1.0, 10.0, H_STEP)
    X = _candidates(sum(PER_SET), seed=n)
    sets = np.repeat(np.arange(len(LENGTHS)), PER_SET).astype(np.int32)
    cand, cand_set = torch.as_tensor(X, device=DEV), torch.as_tensor(sets, device=DEV)
    nb = kernels.step_residual_blocks(max(LENGTHS))

    def launch(Y):
        partial = torch.full((len(Y), nb), SENTINEL, dtype=torch.float64, device=DEV)
        return kernels.step_residual_sets(base, set_begin, max(LENGTHS), torch.as_tensor(Y, device=DEV), cand_set, s, a,
                                          nx, partial=partial)

    value, partial, status = launch(X)
    value2, partial2, _ = launch(X)
    torch.cuda.synchronize()
    assert status.eq(0).all()
    P, v = partial.cpu().numpy(), value.cpu().numpy()
    for j, st in enumerate(sets):
        lo, hi = begin[st], begin[st + 1]
        sl = (s[:, lo:hi].contiguous(), a[:, lo:hi].contiguous(), nx[:, lo:hi].contiguous())
        ref = kernels.step_residual(sw.SwParams.make(n, X[j, 0], X[j, 1], X[j, 2], H_STEP), *sl)
        w = ref.shape[0]
        assert w == kernels.step_residual_blocks(hi - lo)
        assert torch.equal(partial[j, :w], ref), (n, j)
        assert np.all(P[j, w:] == SENTINEL), (n, j)                 # the rest of the row is not written
        assert v[j] == _ordered_sum(P[j, :w]), (n, j)
        pop, _, _ = kernels.step_residual_population(base, cand[j:j + 1].contiguous(), *sl)
        assert v[j] == pop.item(), (n, j)
    assert torch.equal(value, value2) and torch.equal(partial, partial2)        # bit-reproducible

    bad = 12                                                        # inside set 3's run, in the second group
    for row in ([-1.0, 1.0, 10.0], [1.0, 1.0, np.inf]):
        Y = X.copy()
        Y[bad] = row
        vb, pb, stb = launch(Y)
        w = kernels.step_residual_blocks(LENGTHS[sets[bad]])
        assert stb.cpu().tolist() == [0] * bad + [8] + [0] * (len(X) - bad - 1)
        assert torch.isnan(vb[bad]) and torch.isnan(pb[bad, :w]).all() and pb[bad, w:].eq(SENTINEL).all()
        keep = [j for j in range(len(X)) if j != bad]
        assert torch.equal(vb[keep], value[keep]) and torch.equal(pb[keep], partial[keep])


# ---- kernel 2 -----------------------------------------------------------------------------------------------------
def _torch_normal(n, u, s, a, nx):
    """Estimator._residual_normal / _residual_cost on one slice: (r.r, J^T J, J^T r) from kernels.step."""
    def r(v):
        m_i, l_i, k = cmaes.from_constants(v)
        nxt, _ = kernels.step(sw.SwParams.make(n, l_i, m_i, k, H_STEP), s, a)
        return (nxt - nx).reshape(-1)

    r0 = r(u)
    cols = []
    for i in range(3):
        e = np.zeros(3)
        e[i] = 1e-6 * abs(u[i])
        cols.append((r(u + e) - r(u - e)) / (2 * e[i]))
    J = torch.stack(cols)
    return (r0 @ r0).item(), (J @ J.T).cpu().numpy(), (J @ r0).cpu().numpy()


def _points(U, normal):
    """Per set: the centre and, for the normal equations, u +- 1e-6 |u_i| e_i, as (l_i, m_i, k); and 1 / (2 e_i)."""
    pts, inv = [], []
    for u in U:
        row, e_inv = [u], []
        for i in range(3 if normal else 0):
            e = np.zeros(3)
            e[i] = 1e-6 * abs(u[i])
            row += [u + e, u - e]
            e_inv.append(1.0 / (2 * e[i]))
        pts.append([np.array(cmaes.from_constants(v))[[1, 0, 2]] for v in row])
        inv.append(e_inv)
    return (torch.as_tensor(np.array(pts), device=DEV).contiguous(),
            torch.as_tensor(np.array(inv), device=DEV).contiguous() if normal else None)


@pytest.mark.parametrize("n", [2, 3, 6, 8])
def test_normal_equations_per_set_match_the_step_kernel_and_torch(n):
    lengths = [1, 257, 4097]
    s, a, nx, set_begin, begin = _sets(n, lengths, seed=n * 104729)
    base = sw.SwParams.make(n, 1.0, 1.0, 10.0, H_STEP)
    X = _candidates(3, seed=100 + n)                                 # (l_i, m_i, k) per set
    U = [cmaes.to_constants(x[1], x[0], x[2]) for x in X]
    active = torch.as_tensor(np.array([1, 0, 1], dtype=np.int32), device=DEV)
    eps = 2.0 ** -53
    worst = 0.0
    for normal, K in ((True, 13), (False, 1)):
        points, inv_2e = _points(U, normal)

        def launch():
            out = torch.full((3, K), SENTINEL, dtype=torch.float64, device=DEV)
            status = torch.full((3,), 77, dtype=torch.int32, device=DEV)
            return kernels.step_residual_normal_sets(base, set_begin, max(lengths), points, s, a, nx, inv_2e=inv_2e,
                                                     active=active, out=out, status=status)

        out, status = launch()
        out2, _ = launch()
        assert torch.equal(out, out2)                               # bit-reproducible
        got = out.cpu().numpy()
        assert np.all(got[1] == SENTINEL) and status.cpu().tolist() == [0, 77, 0]    # the inactive set is untouched
        for st in (0, 2):
            lo, hi = begin[st], begin[st + 1]
            T = int(hi - lo)
            rr, G, g = _torch_normal(n, U[st], s[:, lo:hi].contiguous(), a[:, lo:hi].contiguous(),
                                     nx[:, lo:hi].contiguous())
            bound = 8 * T * eps
            err, allowed = [abs(got[st, 0] - rr)], [bound * rr]
            if normal:
                d = np.sqrt(np.diag(G))
                err += list(np.abs(got[st, 1:10].reshape(3, 3) - G).ravel()) + list(np.abs(got[st, 10:13] - g))
                allowed += list((bound * np.outer(d, d)).ravel()) + list(bound * d * np.sqrt(rr))
                assert np.array_equal(got[st, 1:10].reshape(3, 3), got[st, 1:10].reshape(3, 3).T)
            ratio = max(e / al for e, al in zip(err, allowed))
            print(f"n={n} T={T} normal={normal}: largest error / allowed = {ratio:.3f}")
            worst = max(worst, ratio)
            assert all(e <= al for e, al in zip(err, allowed)), (n, T, normal, err, allowed)

    # a point that breaks the parameter rule: its set is NaN and flagged, the other set keeps its bits
    points, inv_2e = _points(U, True)
    good, _ = kernels.step_residual_normal_sets(base, set_begin, max(lengths), points, s, a, nx, inv_2e=inv_2e)
    points[2, 3, 1] = -1.0
    out, status = kernels.step_residual_normal_sets(base, set_begin, max(lengths), points, s, a, nx, inv_2e=inv_2e)
    assert status.cpu().tolist() == [0, 0, 8] and torch.isnan(out[2]).all() and torch.equal(out[:2], good[:2])


# ---- EstimatorBatch -----------------------------------------------------------------------------------------------
def _next_rows():
    g = np.load(os.path.join(GOLDEN, "next_rows.npz"))
    db = Database()
    for P, tr in zip(g["est_policies"], g["est_trajectories"]):
        db.add_trajectory(tr.tolist(), P)
    m_i, l_i, k, h = (float(v) for v in g["est_guess"])
    guess = sw.EnvParam("Simulator with estimation", n=3, H=g["est_trajectories"].shape[1], l_i=l_i, m_i=m_i, h=h, k=k,
                        epsilon=0.01)
    return db, guess, g


def _single(db, guess, subset_seed, capacity):
    np.random.seed(subset_seed)
    return Estimator(db, guess, capacity=capacity)


def test_I_population_rows_are_the_single_estimators():
    db, guess, g = _next_rows()
    seeds = [12, 1, 2]
    batch = EstimatorBatch(db, guess, capacity=4, seeds=seeds)
    assert len({sub.tobytes() for sub in batch.subsets}) == 3
    Xs = [g["est_x"], g["est_x"][::-1].copy(), g["est_x"][:2]]
    rows = batch.I_population(Xs)
    for a, (seed, X) in enumerate(zip(seeds, Xs)):
        one = _single(db, guess, seed, 4)
        assert np.array_equal(one.subset, batch.subsets[a])
        assert rows[a].shape == (len(X),) and np.array_equal(rows[a], one.I_population(X)), a
    for got, want in zip(rows[0], g["est_I"]):                      # seed 12 draws the reference's subset
        if want == 0.0:
            assert got < 1e-11
        else:
            assert got == pytest.approx(want, rel=1e-9)
    X = g["est_x"].copy()
    X[1, 0] = -1.0                                                    # m_i < 0
    f = batch.I_population([X, X, X])
    assert all(np.isnan(r[1]) and np.isfinite(r[[0, 2]]).all() for r in f)


def test_lockstep_search_is_the_single_search_bit_for_bit(monkeypatch):
    db, guess, g = _next_rows()
    want = []
    for seed in range(5):
        one = _single(db, guess, 12, 4)
        ep = one.estimate_real_env_param(method="native", seed=seed, refine=False)
        want.append((ep, one.best_f, one.generations, one.evaluations, one.stop_reason))
    batch = EstimatorBatch(db, guess, capacity=4, seeds=[12] * 5)
    assert batch.n_sets == 1 and np.array_equal(batch.subsets[0], g["est_subset"])
    launches = []
    inner = kernels.step_residual_sets

    def counting(*a, **kw):
        launches.append(1)
        return inner(*a, **kw)

    def forbidden(*a, **kw):
        raise AssertionError("the single-candidate objective must not be called by the lock-step search")

    monkeypatch.setattr(kernels, "step_residual_sets", counting)
    monkeypatch.setattr(kernels, "step_residual", forbidden)
    monkeypatch.setattr(kernels, "step_residual_population", forbidden)
    eps = batch.estimate(seeds=list(range(5)), refine=False)
    for a, (ep, best_f, generations, evaluations, stop_reason) in enumerate(want):
        assert eps[a] == ep, (a, eps[a], ep)
        assert (batch.best_f[a], batch.generations[a], batch.evaluations[a], batch.stop_reason[a]) == \
            (best_f, generations, evaluations, stop_reason), a
    assert len(launches) == batch.generations.max()


def test_refined_estimates_recover_the_real_parameters_on_two_stores_in_one_batch(monkeypatch):
    db, guess, g = _next_rows()
    small = Database()
    small.load(os.path.join(GOLDEN, "safe_agent_db.npz"))
    guess20 = sw.EnvParam("Simulator with estimation", n=3, H=20, l_i=1.0, m_i=1.0, k=10.0, h=1e-3, epsilon=0.0)
    drawn = np.random.RandomState(11).randint(0, small.size, 1)     # the rollout the safe-agent cases estimate from
    batch = EstimatorBatch([db] * 5 + [small] * 2, [guess] * 5 + [guess20] * 2, capacity=4,
                           subsets=[g["est_subset"]] * 5 + [drawn] * 2)

    def forbidden(*a, **kw):
        raise AssertionError("the refinement must not launch sw_step_f64")

    monkeypatch.setattr(kernels, "step", forbidden)
    eps = batch.estimate(seeds=[0, 1, 2, 3, 4, 0, 1], refine=True)
    assert len(eps) == 7 and [e.H for e in eps] == [60] * 5 + [20] * 2
    for a, ep in enumerate(eps):
        x = np.array([ep.m_i, ep.l_i, ep.k])
        print(f"estimator {a}: error {np.abs(x - TRUE_X).max():.3e}, best_f {batch.best_f[a]:.3e}, "
              f"{batch.generations[a]} generations, stop {batch.stop_reason[a]}")
    for a, ep in enumerate(eps):
        x = np.array([ep.m_i, ep.l_i, ep.k])
        assert np.abs(x - TRUE_X).max() <= 1e-6, (a, x, batch.stop_reason[a])
        assert batch.best_f[a] < 1e-9, (a, batch.best_f[a])


# ---- the consumer -------------------------------------------------------------------------------------------------
SWEEP = dict(A_values=(0.5,), epsilons=[0.001], n_seed=2, n_iter=2, hand_iter=10, H=20)


def test_sweep_with_computed_simulators(tmp_path):
    guess = sw.EnvParam("Simulator with estimation", n=3, H=20, l_i=1.0, m_i=1.0, k=10.0, h=1e-3, epsilon=0.0)
    out = safe_exploration.run(guess_param=guess, estimator_options={"refine": False}, **SWEEP,
                               results_path=str(tmp_path / "results"), data_path=str(tmp_path / "data"))
    assert out["r_graphs"].shape == (1, 1, 2, 3)
    store = Database()
    store.load(str(tmp_path / "data" / "hand_trajectories.npz"))
    assert store.size > 0 and len(out["sim_params"]) == 2
    for seed, got in enumerate(out["sim_params"]):
        np.random.seed(seed)
        want = Estimator(store, guess, capacity=1).estimate_real_env_param(method="native", seed=seed, refine=False)
        assert got == want, (seed, got, want)


def test_sweep_without_a_guess_is_unchanged(tmp_path):
    g = np.load(os.path.join(GOLDEN, "safe_exploration_small.npz"))
    out = safe_exploration.run(**SWEEP, rng=np.random.RandomState(7), results_path=str(tmp_path / "results"),
                               data_path=str(tmp_path / "data"))
    assert out["r_graphs"].shape == (1, 1, 2, 3)
    assert np.array_equal(out["r_graphs"], g["r_graphs"], equal_nan=True) and out["l"] == float(g["l"])
    sims = safe_exploration.sweep_agents(out["l"], 20, (0.5,), [0.001], 2, 1, 0.001, np.random.RandomState(7))[1]
    assert out["sim_params"] == sims                                # the perturbed simulators, as before
