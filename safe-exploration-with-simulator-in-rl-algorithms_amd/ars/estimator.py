"""Simulator-parameter estimator: mirror of the reference `Estimator` objective functions
(ars/estimator.py:17-87, 112-121).

The reference evaluates its objective I(x) by looping over every stored transition:
`set_state(s)`, `step(select_action(policy, s))`, compare with the stored next state
(estimator.py:50-55) -- an embarrassingly parallel batch of single physics steps.  Here all
transitions of all selected trajectories go through ONE launch that steps every transition AND
compares it with its stored next state (sw_step_residual_f64: the simulated states never reach
memory); J(x) is one launch of the rollout kernel.

The CMA-ES search around I (estimator.py:89-110) asks for a whole generation of candidates at a time, so
I_population(X) scores all of them in ONE launch (sw_step_residual_pop_f64: each stored transition is read once for a
group of candidates) with one host->device copy of the candidates and one device->host read of the values.
estimate_real_env_param(method="native") runs the built-in NumPy CMA-ES (ars/cmaes.py) on it, one launch per
generation; method="cma" keeps the optional `cma` package on I(x); "auto" takes `cma` when it imports.
"""
import dataclasses
import math

import numpy as np
import torch

from .. import kernels
from .._lib import SwParams, require_gpu
from . import cmaes
from .parameters import EnvParam


class Estimator(object):

    def __init__(self, database, guess_param, capacity, unknowns=('m_i', 'l_i', 'k'),
                 device="cuda:0", subset=None):
        """subset: the rollouts to estimate from, instead of `capacity` draws from NumPy's global generator (which
        is then not touched; EstimatorBatch draws its estimators' subsets from generators of their own)."""
        assert database.size > 0, "Database is empty"
        if database._device_batches and not database._trajectories:   # still on the GPU: keep it there
            assert database._device_batches[0][0].shape[0] == guess_param.H, "Rollouts are not the same"
        else:
            assert len(database.trajectories[0]) == guess_param.H, "Rollouts are not the same"
        self.guess_param = guess_param
        self.unknowns = unknowns
        self.database = database
        self.subset = (np.random.randint(0, self.database.size, capacity) if subset is None   # estimator.py:33
                       else np.asarray(subset, dtype=np.int64))
        self.iter = 0
        self.device = torch.device(device)
        self._cache = None
        self._partial = None
        self._jcache = None
        self._pop = None
        self.generations = self.evaluations = 0
        self.best_f = self.stop_reason = None

    def convert_to_env_param(self, x):
        d = dataclasses.asdict(self.guess_param)
        for i in range(len(self.unknowns)):
            d[self.unknowns[i]] = x[i]
        return EnvParam(**d)

    def _params(self, x):
        ep = self.convert_to_env_param(x)
        return SwParams.make(ep.n, ep.l_i, ep.m_i, ep.k, ep.h, (1.0, 0.0))

    def _batch_from_device_store(self):
        """The same batch straight from a store that is still on the GPU (the rollout kernels'
        [H, d, R] tensors, Database.add_device_batch): no host round trip, no per-rollout loop.
        Transitions are grouped by iteration batch instead of by subset order (I(x) is a sum)."""
        db = self.database
        sizes = np.array([t.shape[2] for t, _ in db._device_batches])
        first = np.concatenate(([0], np.cumsum(sizes)))
        which = np.searchsorted(first, self.subset, side="right") - 1
        S, Nx, A, lens = [], [], [], []
        for b, (traj, pols) in enumerate(db._device_batches):
            cols = self.subset[which == b] - first[b]
            if cols.size == 0:
                continue
            idx = torch.as_tensor(cols, device=self.device)
            tr = traj.to(self.device).index_select(2, idx)                # [H, d, c]
            s = tr[:-1].permute(1, 2, 0).reshape(tr.shape[1], -1)           # [d, c * (H-1)], rollout-major
            nx = tr[1:].permute(1, 2, 0).reshape(tr.shape[1], -1)
            P = torch.as_tensor(np.ascontiguousarray(np.asarray(pols, dtype=np.float64)[cols]),
                                device=self.device)                          # [c, m, d]
            a = torch.einsum("cmd,tdc->mct", P, tr[:-1]).reshape(P.shape[1], -1)
            S.append(s)
            Nx.append(nx)
            A.append(a)
            lens += [tr.shape[0] - 1] * cols.size
        return (torch.cat(S, 1).contiguous(), torch.cat(Nx, 1).contiguous(),
                torch.cat(A, 1).contiguous(), lens)

    def _batch(self):
        """Device copies of the selected trajectories: states [d, T], next states [d, T],
        actions [m, T] (V1 action a = P s, estimator.py:52), segment lengths."""
        if self._cache is None:
            require_gpu()
            db = self.database
            if db._device_batches and not db._trajectories:
                self._cache = self._batch_from_device_store()
                return self._cache
            S, Nx, A, lens = [], [], [], []
            for k in self.subset:
                P = torch.as_tensor(np.asarray(self.database.policies[k], dtype=np.float64),
                                    device=self.device)
                tr = torch.as_tensor(np.asarray(self.database.trajectories[k], dtype=np.float64),
                                     device=self.device)
                s, nx = tr[:-1].T.contiguous(), tr[1:].T.contiguous()
                S.append(s)
                Nx.append(nx)
                A.append(P @ s)
                lens.append(s.shape[1])
            self._cache = (torch.cat(S, 1).contiguous(), torch.cat(Nx, 1).contiguous(),
                           torch.cat(A, 1).contiguous(), lens)
        return self._cache

    def I(self, x):
        """Sum over stored transitions of || sim_step(s_t, a_t) - s_{t+1} ||_2."""
        states, nexts, actions, _ = self._batch()
        # one pass: step + distance to the stored next state + per-workgroup sums (sw_step_residual_f64); the
        # simulated states are never written, only T / 256 partial sums are
        if self._partial is None or self._partial.shape[0] != kernels.step_residual_blocks(states.shape[1]):
            self._partial = torch.empty(kernels.step_residual_blocks(states.shape[1]), dtype=torch.float64,
                                        device=self.device)
        kernels.step_residual(self._params(x), states, actions, nexts, partial=self._partial)
        return float(self._partial.sum().item())

    def J(self, x):
        """Deprecated objective of the reference (estimator.py:64-87): whole-rollout distance.  ONE launch of the
        rollout kernels over every selected rollout (the reference re-runs them one after the other), then the
        per-step and per-rollout norms on the device."""
        require_gpu()
        p = self._params(x)
        if self._jcache is None:
            P = np.stack([np.asarray(self.database.policies[k], dtype=np.float64) for k in self.subset])
            real = np.stack([np.asarray(self.database.trajectories[k], dtype=np.float64) for k in self.subset])
            self._jcache = (torch.as_tensor(P, device=self.device).contiguous(),
                            torch.as_tensor(real, device=self.device).permute(1, 2, 0).contiguous())   # [H, d, K]
        P, real = self._jcache
        H, K = real.shape[0], real.shape[2]
        traj = torch.empty((H, p.d, K), dtype=torch.float64, device=self.device)
        kernels.rollout(p, H, P, traj=traj)
        per_step = torch.linalg.vector_norm(traj - real, ord=2, dim=1)             # [H, K]
        dists = torch.linalg.vector_norm(per_step, ord=2, dim=0) / H               # [K]
        return float(dists.mean().item())

    def feasible(self, x):
        """The parameter rule of the library (validate_params): l_i, m_i positive and finite, k finite."""
        ep = self.convert_to_env_param(x)
        return (ep.l_i > 0 and ep.m_i > 0 and math.isfinite(ep.l_i) and math.isfinite(ep.m_i)
                and math.isfinite(ep.k))

    def I_population(self, X):
        """I(x) for every row of X [lambda, len(unknowns)] -> NumPy [lambda]: one host->device copy of the
        candidates, ONE launch (sw_step_residual_pop_f64), one device->host read of the values and status.  A row
        that breaks the parameter rule scores NaN."""
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        if X.shape[1] != len(self.unknowns):
            raise ValueError(f"expected rows of {len(self.unknowns)} unknowns, got shape {X.shape}")
        states, nexts, actions, _ = self._batch()
        eps = [self.convert_to_env_param(x) for x in X]
        cand = np.array([[ep.l_i, ep.m_i, ep.k] for ep in eps], dtype=np.float64)
        g = self.guess_param
        base = SwParams.make(g.n, g.l_i, g.m_i, g.k, g.h, (1.0, 0.0))   # n, h, direction; l_i, m_i, k per candidate
        lam, nb = cand.shape[0], kernels.step_residual_blocks(states.shape[1])
        if self._pop is None or self._pop[0].shape[0] != lam or self._pop[1].shape[1] != nb:
            self._pop = (torch.zeros(lam, dtype=torch.float64, device=self.device),
                         torch.empty((lam, nb), dtype=torch.float64, device=self.device),
                         torch.zeros(lam, dtype=torch.int32, device=self.device),
                         torch.empty((lam, 3), dtype=torch.float64, pin_memory=True))
        value, partial, status, host = self._pop
        host.numpy()[:] = cand
        dcand = host.to(self.device, non_blocking=True)
        kernels.step_residual_population(base, dcand, states, actions, nexts, partial=partial, value=value,
                                         status=status)
        out = torch.cat((value, status.to(torch.float64))).cpu().numpy()
        f = out[:lam].copy()
        f[out[lam:] != 0] = np.nan
        return f

    def _residual_normal(self, u):
        """Per-transition residuals r = step(x(u)) - stored next state, u = (k l / m, m l^2, k / m): (r.r, J^T J, J^T r)
        with J by central differences in u (seven step launches, the reductions on the device, one read)."""
        states, nexts, actions, _ = self._batch()
        g = self.guess_param

        def r(v):
            m_i, l_i, k = cmaes.from_constants(v)
            nxt, _ = kernels.step(SwParams.make(g.n, l_i, m_i, k, g.h, (1.0, 0.0)), states, actions)
            return (nxt - nexts).reshape(-1)

        r0 = r(u)
        cols = []
        for i in range(3):
            e = np.zeros(3)
            e[i] = 1e-6 * abs(u[i])
            cols.append((r(u + e) - r(u - e)) / (2 * e[i]))
        J = torch.stack(cols)                                                       # [3, d T]
        out = torch.cat(((r0 @ r0).reshape(1), (J @ J.T).reshape(-1), J @ r0)).cpu().numpy()
        return out[1:10].reshape(3, 3), out[10:]

    def _residual_cost(self, u):
        states, nexts, actions, _ = self._batch()
        g = self.guess_param
        m_i, l_i, k = cmaes.from_constants(u)
        nxt, _ = kernels.step(SwParams.make(g.n, l_i, m_i, k, g.h, (1.0, 0.0)), states, actions)
        return float(((nxt - nexts) ** 2).sum().item())

    def _refine(self, x):
        """Least-squares refinement of the search's best point in the model's constants (cmaes.refine_least_squares);
        kept only when I is lower there."""
        idx = [list(self.unknowns).index(n) for n in ("m_i", "l_i", "k")]
        u = cmaes.refine_least_squares(self._residual_cost, self._residual_normal,
                                       cmaes.to_constants(*np.asarray(x)[idx]), feasible=lambda v: bool(np.all(v > 0)))
        xr = np.empty(3)
        xr[idx] = cmaes.from_constants(u)
        fr = self.I_population([xr])[0]
        if fr < self.best_f:
            self.best_f = float(fr)
            return xr
        return np.asarray(x)

    def estimate_real_env_param(self, method="auto", seed=0, sigma0=1.0, popsize=None, max_generations=None,
                                refine=True):
        """CMA-ES over I(x) (estimator.py:89-110), starting at the guess with sigma0 = 1.
        method "cma": the optional `cma` package on I(x), one launch per candidate; "native": the built-in search
        (ars/cmaes.py, seeded by `seed`) on I_population, one launch per generation; "auto": "cma" when it imports,
        else "native".  The native search keeps generations, evaluations, best_f and stop_reason on the estimator and,
        when the unknowns are m_i, l_i and k and `refine` is set, refines its best point by least squares on the
        per-transition residuals (cmaes.refine_least_squares, in the constants k l / m, m l^2, k / m)."""
        if method not in ("auto", "cma", "native"):
            raise ValueError(f"method must be 'auto', 'cma' or 'native', not {method!r}")
        if method == "auto":
            try:
                import cma
                method = "cma" if hasattr(cma, "CMAEvolutionStrategy") else "native"
            except ImportError:
                method = "native"
        print("------ Estimating the real world environment parameters ------")
        print("Extracting the initial guess of real world parameters...")
        d = dataclasses.asdict(self.guess_param)
        x0 = np.array([d[u] for u in self.unknowns], dtype=np.float64)
        print(f"Initial estimation extracted: {x0}")
        print("Starting estimation...")
        if method == "cma":
            import cma
            es = cma.CMAEvolutionStrategy(x0, 1).optimize(self.I)
            est_x, _, _ = es.best.get()
        else:
            es = cmaes.minimize(self.I_population, x0, sigma0=sigma0, popsize=popsize, seed=seed,
                                feasible=self.feasible, max_generations=max_generations)
            est_x, self.best_f = es.best_x, es.best_f
            self.generations, self.evaluations, self.stop_reason = es.generations, es.evaluations, es.stop_reason
            print(f"native CMA-ES: best f {es.best_f:.6e} at {est_x}, {es.generations} generations, "
                  f"{es.evaluations} evaluations, stop: {es.stop_reason}")
            if refine and sorted(self.unknowns) == ["k", "l_i", "m_i"] and np.isfinite(es.best_f):
                est_x = self._refine(est_x)
                print(f"refined: f {self.best_f:.6e} at {est_x}")
        print("Estimation finished")
        env_param = self.convert_to_env_param(est_x)
        print(f"Estimated parameters: {env_param}")
        return env_param
