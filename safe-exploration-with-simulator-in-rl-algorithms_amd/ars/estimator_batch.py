"""Many simulator-parameter estimates in lock-step: `Estimator.estimate_real_env_param(method="native")` (reference
ars/estimator.py:89-110 behind ars/ars_agent.py:40-44) for a batch of estimators, with one launch per CMA-ES generation
for ALL of them instead of one per estimator.

The searches are independent, and one estimator's launch (a few hundred to a few thousand stored transitions times a
handful of candidates) is far too small to fill the chip.  Here every estimator's transitions are one SET of columns
of one concatenated batch; per generation every live search asks for its candidates, ONE launch of
sw_step_residual_sets_f64 scores each candidate on its estimator's set -- with the bits `Estimator.I_population` gives
-- and every search is told (cmaes.minimize_many).  The least-squares refinement runs in lock-step too
(cmaes.refine_least_squares_many) over sw_step_residual_normal_sets_f64, which forms r.r, J^T J and J^T r per set in
one launch; the seven step launches and the torch reductions of `Estimator._residual_normal` do not happen, and the
simulated states never reach memory.

Estimator a is, for the search, exactly `np.random.seed(seeds[a]); Estimator(databases[a], guess_params[a], capacity)`
followed by `estimate_real_env_param(method="native", seed=..., refine=False)`: same subset, same candidates, same
values, same stop.  The refinement sums the same per-transition terms in another order, so a refined estimate agrees
with the single estimator's to rounding, not bit for bit.  Only the built-in search is offered: the `cma` package draws
from the clock and cannot be stepped in lock-step reproducibly.
"""
import dataclasses
import math

import numpy as np
import torch

from .. import kernels
from .._lib import SwParams
from . import cmaes
from .estimator import Estimator
from .parameters import EnvParam

_KERNEL_FIELDS = ("l_i", "m_i", "k")      # the columns of the kernels' candidates


class EstimatorBatch(object):

    def __init__(self, databases, guess_params, capacity, seeds=None, subsets=None, unknowns=('m_i', 'l_i', 'k'),
                 device="cuda:0"):
        """databases / guess_params: one object for all estimators or one per estimator.  subsets[a] (indices into
        the store) is given, or drawn as np.random.RandomState(seeds[a]).randint(0, size, capacity) -- the subset
        `np.random.seed(seeds[a]); Estimator(...)` gets; NumPy's global generator is not touched.  No device work
        happens here."""
        counts = {len(v) for v in (databases, guess_params, seeds, subsets) if isinstance(v, (list, tuple, np.ndarray))
                  and not isinstance(v, EnvParam)}
        if len(counts) > 1:
            raise ValueError(f"databases, guess_params, seeds and subsets disagree on the number of estimators: {counts}")
        if seeds is None and subsets is None:
            raise ValueError("give seeds (the subsets are drawn from them) or subsets")
        n = self.n_estimators = counts.pop() if counts else 1
        if n < 1:
            raise ValueError("at least one estimator is required")
        is_db = lambda v: hasattr(v, "add_trajectory")   # noqa: E731
        self.databases = list(databases) if not is_db(databases) else [databases] * n
        self.guess_params = [guess_params] * n if isinstance(guess_params, EnvParam) else list(guess_params)
        self.seeds = None if seeds is None else [int(s) for s in seeds]
        self.unknowns = tuple(unknowns)
        if not self.unknowns or any(u not in _KERNEL_FIELDS for u in self.unknowns):
            raise ValueError(f"unknowns must be taken from {_KERNEL_FIELDS}, not {self.unknowns}")
        self.device = torch.device(device)
        g0 = self.guess_params[0]
        if any(g.n != g0.n or g.h != g0.h for g in self.guess_params):
            raise ValueError("all guesses must share n and h")
        self.subsets = []
        for a in range(n):
            db = self.databases[a]
            assert db.size > 0, "Database is empty"
            if subsets is not None:
                sub = np.asarray(subsets[a], dtype=np.int64).ravel()
                if sub.size < 1 or sub.min() < 0 or sub.max() >= db.size:
                    raise ValueError(f"subsets[{a}]: expected indices into a store of {db.size} rollouts")
            else:
                sub = np.random.RandomState(self.seeds[a]).randint(0, db.size, capacity)
            self.subsets.append(sub)
        # estimators on the same store with equal subsets share one transition set; each set has an internal
        # Estimator that builds its transitions exactly as Estimator._batch() does
        self._set_estimators, self.set_of, index = [], [], {}
        for a in range(n):
            key = (id(self.databases[a]), self.guess_params[a].H, self.subsets[a].tobytes())
            if key not in index:
                index[key] = len(self._set_estimators)
                self._set_estimators.append(Estimator(self.databases[a], self.guess_params[a], capacity,
                                                      unknowns=self.unknowns, device=device,
                                                      subset=self.subsets[a]))
            self.set_of.append(index[key])
        self.n_sets = len(self._set_estimators)
        self._base = SwParams.make(g0.n, g0.l_i, g0.m_i, g0.k, g0.h, (1.0, 0.0))   # n, h, direction
        self._guess_lmk = np.array([[getattr(g, f) for f in _KERNEL_FIELDS] for g in self.guess_params], dtype=np.float64)
        self._guess_rows = [tuple(float(v) for v in row) for row in self._guess_lmk]
        self._columns = [_KERNEL_FIELDS.index(u) for u in self.unknowns]
        self._cache = None
        self.generations = np.zeros(n, dtype=np.int64)
        self.evaluations = np.zeros(n, dtype=np.int64)
        self.best_f = np.full(n, np.nan)
        self.stop_reason = [None] * n

    # ---- the transition sets ----------------------------------------------------------------------------------
    def _sets(self):
        """(states [d, T], next states [d, T], actions [m, T], set_begin int64 [n_sets + 1] on the device, the sets'
        lengths on the host): every set's transitions side by side."""
        if self._cache is None:
            parts = [e._batch() for e in self._set_estimators]
            lens = np.array([p[0].shape[1] for p in parts], dtype=np.int64)
            begin = np.concatenate(([0], np.cumsum(lens)))
            self._cache = (torch.cat([p[0] for p in parts], 1).contiguous(),
                           torch.cat([p[1] for p in parts], 1).contiguous(),
                           torch.cat([p[2] for p in parts], 1).contiguous(),
                           torch.as_tensor(begin, device=self.device), lens)
        return self._cache

    def convert_to_env_param(self, a, x):
        d = dataclasses.asdict(self.guess_params[a])
        for name, v in zip(self.unknowns, x):
            d[name] = v
        return EnvParam(**d)

    def feasible(self, a, x):
        """The parameter rule of the library, as Estimator.feasible (plain floats: the searches call it for every
        point they draw)."""
        v = list(self._guess_rows[a])
        for c, xi in zip(self._columns, x):
            v[c] = xi
        return bool(v[0] > 0 and v[1] > 0 and math.isfinite(v[0]) and math.isfinite(v[1]) and math.isfinite(v[2]))

    # ---- the objective ----------------------------------------------------------------------------------------
    def _score(self, idx, Xs):
        """I(x) for the rows of Xs[j], on estimator idx[j]'s transitions: one copy of all candidates, ONE launch
        (sw_step_residual_sets_f64), one read."""
        if len(idx) != len(Xs):
            raise ValueError(f"{len(Xs)} candidate arrays for {len(idx)} estimators")
        nu = len(self.unknowns)
        Xs = [np.asarray(X, dtype=np.float64).reshape(-1, nu) for X in Xs]
        order = sorted(range(len(idx)), key=lambda j: self.set_of[idx[j]])      # a set's candidates are contiguous
        lam = [Xs[j].shape[0] for j in order]
        total = int(sum(lam))
        out = [np.empty(0)] * len(idx)
        if total == 0:
            return out
        states, nexts, actions, set_begin, lens = self._sets()
        host = torch.empty((total, 4), dtype=torch.float64, pin_memory=True)      # (l_i, m_i, k, set)
        h = host.numpy()
        h[:, :3] = np.repeat(self._guess_lmk[[idx[j] for j in order]], lam, axis=0)   # the guesses' other fields
        h[:, self._columns] = np.concatenate([Xs[j] for j in order])
        h[:, 3] = np.repeat([self.set_of[idx[j]] for j in order], lam)
        dev = host.to(self.device, non_blocking=True)
        cand, cand_set = dev[:, :3].contiguous(), dev[:, 3].to(torch.int32)
        value, _, status = kernels.step_residual_sets(self._base, set_begin, int(lens.max()), cand, cand_set, states,
                                                      actions, nexts)
        got = torch.cat((value, status.to(torch.float64))).cpu().numpy()
        f = got[:total].copy()
        f[got[total:] != 0] = np.nan
        at = 0
        for j, n in zip(order, lam):
            out[j] = f[at:at + n]
            at += n
        return out

    def I_population(self, Xs):
        """Xs[a] [lambda_a, len(unknowns)] -> [lambda_a] values of I on estimator a's transitions, for every
        estimator at once.  A row that breaks the parameter rule scores NaN."""
        if len(Xs) != self.n_estimators:
            raise ValueError(f"expected {self.n_estimators} candidate arrays, got {len(Xs)}")
        for X in Xs:
            X = np.asarray(X)
            if X.size and (X.ndim != 2 or X.shape[1] != len(self.unknowns)):
                raise ValueError(f"expected rows of {len(self.unknowns)} unknowns, got shape {X.shape}")
        return self._score(list(range(self.n_estimators)), Xs)

    # ---- the refinement ---------------------------------------------------------------------------------------
    def _normal_sets(self, idx, U, normal):
        """r.r (normal False) or (r.r, J^T J, J^T r) at U[j] = (k l / m, m l^2, k / m) of estimator idx[j], by
        sw_step_residual_normal_sets_f64: one launch serves one estimator per transition set, so a call is ONE launch
        unless estimators share a set (then one launch per sharer).  The points are Estimator._residual_normal's:
        u and u +- 1e-6 |u_i| e_i."""
        states, nexts, actions, set_begin, lens = self._sets()
        n_point, K = (7, 13) if normal else (1, 1)
        result, todo = [None] * len(idx), list(range(len(idx)))
        while todo:
            taken, later = {}, []
            for j in todo:
                if taken.setdefault(self.set_of[idx[j]], j) != j:
                    later.append(j)
            host = torch.zeros((self.n_sets, 3 * n_point + 4), dtype=torch.float64, pin_memory=True)
            h = host.numpy()
            h[:, :3 * n_point] = 1.0                    # sets without a point this round: valid numbers, never read
            for s, j in taken.items():
                u = np.asarray(U[j], dtype=np.float64)
                pts = [u]
                for i in range(3 if normal else 0):
                    e = np.zeros(3)
                    e[i] = 1e-6 * abs(u[i])
                    pts += [u + e, u - e]
                    h[s, 3 * n_point + i] = 1.0 / (2 * e[i]) if e[i] != 0 else np.inf
                for p, v in enumerate(pts):
                    m_i, l_i, k = cmaes.from_constants(v)
                    h[s, 3 * p:3 * p + 3] = (l_i, m_i, k)
                h[s, 3 * n_point + 3] = 1.0
            dev = host.to(self.device, non_blocking=True)
            points = dev[:, :3 * n_point].contiguous().reshape(self.n_sets, n_point, 3)
            inv_2e = dev[:, 3 * n_point:3 * n_point + 3].contiguous() if normal else None
            active = dev[:, 3 * n_point + 3].to(torch.int32)
            out, _ = kernels.step_residual_normal_sets(self._base, set_begin, int(lens.max()), points, states, actions,
                                                       nexts, inv_2e=inv_2e, active=active,
                                                       out=torch.full((self.n_sets, K), float("nan"),
                                                                      dtype=torch.float64, device=self.device))
            got = out.cpu().numpy()
            for s, j in taken.items():
                result[j] = (got[s, 1:10].reshape(3, 3).copy(), got[s, 10:13].copy()) if normal else float(got[s, 0])
            todo = later
        return result

    def _refine(self, xs):
        """Least-squares refinement of every finite best point, in lock-step; a refined point is kept only where I
        is lower."""
        pos = [self.unknowns.index(f) for f in ("m_i", "l_i", "k")]
        idx = [a for a in range(self.n_estimators) if np.isfinite(self.best_f[a])]
        if not idx:
            return xs
        U0 = [cmaes.to_constants(*np.asarray(xs[a])[pos]) for a in idx]
        U = cmaes.refine_least_squares_many(lambda ii, V: self._normal_sets([idx[i] for i in ii], V, False),
                                            lambda ii, V: self._normal_sets([idx[i] for i in ii], V, True),
                                            U0, feasible=lambda v: bool(np.all(v > 0)))
        XR = []
        for u in U:
            xr = np.empty(3)
            xr[pos] = cmaes.from_constants(u)
            XR.append(xr)
        fr = self._score(idx, [x[None, :] for x in XR])
        xs = list(xs)
        for a, xr, f in zip(idx, XR, fr):
            if f[0] < self.best_f[a]:
                self.best_f[a] = float(f[0])
                xs[a] = xr
        return xs

    # ---- the search -------------------------------------------------------------------------------------------
    def estimate(self, method="native", seeds=None, sigma0=1.0, popsize=None, max_generations=None, refine=True):
        """Every estimator's estimate_real_env_param(method="native", seed=seeds[a], ...) in lock-step -> a list of
        EnvParam.  seeds: the searches' seeds; default the constructor's seeds, else 0 for every estimator.  Keeps
        generations, evaluations, best_f (arrays) and stop_reason (a list) per estimator."""
        if method != "native":
            raise ValueError(f"method must be 'native' (the cma package cannot be stepped in lock-step reproducibly), "
                             f"not {method!r}")
        n = self.n_estimators
        if seeds is None:
            seeds = self.seeds if self.seeds is not None else [0] * n
        if len(seeds) != n:
            raise ValueError(f"expected {n} seeds, got {len(seeds)}")
        x0s = [np.array([dataclasses.asdict(g)[u] for u in self.unknowns], dtype=np.float64) for g in self.guess_params]
        feasibles = [(lambda x, a=a: self.feasible(a, x)) for a in range(n)]
        es = cmaes.minimize_many(self._score, x0s, sigma0=sigma0, popsize=popsize, seeds=list(seeds),
                                 feasibles=feasibles, max_generations=max_generations)
        xs = [e.best_x for e in es]
        self.generations = np.array([e.generations for e in es], dtype=np.int64)
        self.evaluations = np.array([e.evaluations for e in es], dtype=np.int64)
        self.best_f = np.array([e.best_f for e in es], dtype=np.float64)
        self.stop_reason = [e.stop_reason for e in es]
        if refine and sorted(self.unknowns) == ["k", "l_i", "m_i"]:
            xs = self._refine(xs)
        return [self.convert_to_env_param(a, x) for a, x in enumerate(xs)]
