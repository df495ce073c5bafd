"""A plain (mu/mu_w, lambda)-CMA-ES, ask/tell, in NumPy: the search of Estimator.estimate_real_env_param without the
optional `cma` package.

Parameters are the defaults of N. Hansen, "The CMA Evolution Strategy: A Tutorial" (2016), Table 1: lambda =
4 + floor(3 ln N), mu = floor(lambda / 2), positive log weights, c_sigma, d_sigma, c_c, c_1, c_mu and h_sigma as given
there, the eigendecomposition of C every generation.  Stopping follows the `cma` package's defaults:

  tolfun 1e-11        the range of this generation's values and of the best values of the last
                      10 + ceil(30 N / lambda) generations
  tolx 1e-11          sigma * max(|p_c|_inf, max sqrt(diag C))
  conditioncov 1e14   condition number of C
  maxiter             100 + 150 (N + 3)^2 / sqrt(lambda)

Differences from `cma` (whose estimate the reference seeds from the clock, so it cannot be reproduced anyway): no
active (negative-weight) covariance update, a different random stream (its own PCG64 generator; NumPy's global legacy
generator is never touched), and only the stopping rules above.  Candidates that break the caller's `feasible` rule
are redrawn before they are scored, up to 100 times, and score +inf after that; NaN / inf values rank last and ties
go to the lower candidate index.  `best_x` is the best point ever evaluated, as `cma`'s es.best.get().
"""
import math

import numpy as np

TOLFUN = 1e-11
TOLX = 1e-11
MAX_CONDITION = 1e14
MAX_REDRAWS = 100


class CMAES(object):

    def __init__(self, x0, sigma0=1.0, popsize=None, seed=0, feasible=None, max_generations=None, tolfun=TOLFUN,
                 tolx=TOLX):
        self.mean = np.array(x0, dtype=np.float64).ravel()
        N = self.N = self.mean.size
        if N < 1:
            raise ValueError("x0 must have at least one coordinate")
        if not sigma0 > 0:
            raise ValueError("sigma0 must be positive")
        self.sigma = float(sigma0)
        self.lam = int(popsize) if popsize is not None else 4 + int(math.floor(3 * math.log(N)))
        if self.lam < 2:
            raise ValueError("popsize must be at least 2")
        self.mu = self.lam // 2
        w = math.log((self.lam + 1) / 2.0) - np.log(np.arange(1, self.mu + 1))
        self.weights = w / w.sum()
        self.mueff = 1.0 / np.sum(self.weights ** 2)
        mueff = self.mueff
        self.cs = (mueff + 2) / (N + mueff + 5)
        self.damps = 1 + 2 * max(0.0, math.sqrt((mueff - 1) / (N + 1)) - 1) + self.cs
        self.cc = (4 + mueff / N) / (N + 4 + 2 * mueff / N)
        alpha_cov = 2.0
        self.c1 = alpha_cov / ((N + 1.3) ** 2 + mueff)
        self.cmu = min(1 - self.c1, alpha_cov * (mueff - 2 + 1 / mueff) / ((N + 2) ** 2 + alpha_cov * mueff / 2))
        self.chiN = math.sqrt(N) * (1 - 1 / (4 * N) + 1 / (21 * N * N))
        self.max_generations = (int(max_generations) if max_generations is not None
                                else int(100 + 150 * (N + 3) ** 2 / math.sqrt(self.lam)))
        self.hist_len = 10 + int(math.ceil(30 * N / self.lam))
        self.tolfun, self.tolx = float(tolfun), float(tolx)

        self.pc = np.zeros(N)
        self.ps = np.zeros(N)
        self.C = np.eye(N)
        self.B = np.eye(N)
        self.D = np.ones(N)
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.feasible = feasible
        self.generations = 0
        self.evaluations = 0
        self.best_x, self.best_f = self.mean.copy(), math.inf
        self._best_hist = []         # best value of each generation, newest last
        self._last_f = None
        self.stop_reason = None

    def _sample(self):
        return self.mean + self.sigma * (self.B @ (self.D * self.rng.standard_normal(self.N)))

    def ask(self):
        """The next generation, [lambda, N]; a point the `feasible` rule refuses is redrawn up to 100 times."""
        X = np.empty((self.lam, self.N))
        for i in range(self.lam):
            x = self._sample()
            if self.feasible is not None:
                tries = 0
                while not self.feasible(x) and tries < MAX_REDRAWS:
                    x = self._sample()
                    tries += 1
            X[i] = x
        return X

    def tell(self, X, f):
        X = np.asarray(X, dtype=np.float64)
        f = np.asarray(f, dtype=np.float64).ravel()
        if X.shape != (self.lam, self.N) or f.shape != (self.lam,):
            raise ValueError(f"expected {self.lam} candidates of dimension {self.N} and {self.lam} values")
        key = np.where(np.isnan(f), np.inf, f)
        order = np.argsort(key, kind="stable")        # NaN / inf last, ties by candidate index
        self.evaluations += self.lam
        self.generations += 1
        if key[order[0]] < self.best_f:
            self.best_f, self.best_x = float(key[order[0]]), X[order[0]].copy()
        self._best_hist.append(float(key[order[0]]))
        self._last_f = key[order]

        N, old = self.N, self.mean
        Y = (X[order[:self.mu]] - old) / self.sigma            # y_{i:lambda}
        yw = self.weights @ Y
        self.mean = old + self.sigma * yw
        invsqrtC = self.B @ np.diag(1.0 / self.D) @ self.B.T
        self.ps = (1 - self.cs) * self.ps + math.sqrt(self.cs * (2 - self.cs) * self.mueff) * (invsqrtC @ yw)
        ps_norm = float(np.linalg.norm(self.ps))
        hsig = ps_norm / math.sqrt(1 - (1 - self.cs) ** (2 * self.generations)) < (1.4 + 2 / (N + 1)) * self.chiN
        self.pc = (1 - self.cc) * self.pc + (math.sqrt(self.cc * (2 - self.cc) * self.mueff) * yw if hsig else 0.0)
        dh = 0.0 if hsig else self.cc * (2 - self.cc)
        rank_mu = (Y.T * self.weights) @ Y
        self.C = ((1 + self.c1 * dh - self.c1 - self.cmu * self.weights.sum()) * self.C
                  + self.c1 * np.outer(self.pc, self.pc) + self.cmu * rank_mu)
        self.sigma *= math.exp((self.cs / self.damps) * (ps_norm / self.chiN - 1))
        self.C = (self.C + self.C.T) / 2
        ev, self.B = np.linalg.eigh(self.C)
        self.D = np.sqrt(np.maximum(ev, 0.0))

    def stop(self):
        """The name of the first stopping rule that holds, or None."""
        if self.generations >= self.max_generations:
            self.stop_reason = "maxiter"
        elif (self.generations >= self.hist_len and np.all(np.isfinite(self._last_f))
              and self._last_f[-1] - self._last_f[0] < self.tolfun
              and max(self._best_hist[-self.hist_len:]) - min(self._best_hist[-self.hist_len:]) < self.tolfun):
            self.stop_reason = "tolfun"
        elif self.sigma * max(np.abs(self.pc).max(), np.sqrt(np.diag(self.C)).max()) < self.tolx:
            self.stop_reason = "tolx"
        elif self.D.min() <= 0 or (self.D.max() / self.D.min()) ** 2 > MAX_CONDITION:
            self.stop_reason = "conditioncov"
        return self.stop_reason


def minimize(fun_population, x0, sigma0=1.0, popsize=None, seed=0, feasible=None, max_generations=None,
             tolfun=TOLFUN, tolx=TOLX):
    """Run the search to its stop: `fun_population(X)` scores a whole generation X [lambda, N] -> [lambda] (one call
    per generation).  Points the `feasible` rule still refuses after the redraws are scored +inf without being passed
    to it.  Returns the CMAES object (best_x, best_f, generations, evaluations, stop_reason)."""
    es = CMAES(x0, sigma0, popsize=popsize, seed=seed, feasible=feasible, max_generations=max_generations,
               tolfun=tolfun, tolx=tolx)
    while es.stop() is None:
        X = es.ask()
        ok = np.ones(es.lam, dtype=bool) if feasible is None else np.array([bool(feasible(x)) for x in X])
        f = np.full(es.lam, np.inf)
        if ok.any():
            f[ok] = np.asarray(fun_population(X[ok]), dtype=np.float64).ravel()
        es.tell(X, f)
    return es


def minimize_many(fun_many, x0s, sigma0=1.0, popsize=None, seeds=None, feasibles=None, max_generations=None,
                  tolfun=TOLFUN, tolx=TOLX):
    """`minimize` for many independent searches in lock-step: one CMAES object per row of x0s, each with its own
    generator (seeds[i]; default 0 for every instance).  Per generation every live instance asks, `fun_many(idx, Xs)`
    is called ONCE -- idx the indices of the live instances, Xs[j] the points of instance idx[j] that its `feasible`
    rule accepts (an empty array when it accepts none; the refused ones score +inf as in `minimize`) -> one array of
    values per entry of Xs -- and every live instance is told.  An instance that stops drops out; the loop ends when
    none is live.  sigma0, popsize, feasibles and max_generations are one value for all or a list with one per
    instance.  Returns the list of CMAES objects; instance i ends exactly where minimize(fun_i, x0s[i], seed=seeds[i],
    ...) ends."""
    n = len(x0s)

    def per(v, kind):
        return list(v) if isinstance(v, kind) else [v] * n

    sigma0, popsize = per(sigma0, (list, tuple, np.ndarray)), per(popsize, (list, tuple, np.ndarray))
    feasibles, max_generations = per(feasibles, (list, tuple)), per(max_generations, (list, tuple, np.ndarray))
    seeds = [0] * n if seeds is None else list(seeds)
    if not all(len(v) == n for v in (sigma0, popsize, feasibles, max_generations, seeds)):
        raise ValueError(f"expected one value or {n} values per argument")
    es = [CMAES(x0s[i], sigma0[i], popsize=popsize[i], seed=seeds[i], feasible=feasibles[i],
                max_generations=max_generations[i], tolfun=tolfun, tolx=tolx) for i in range(n)]
    live = [i for i in range(n) if es[i].stop() is None]
    while live:
        Xs, oks = [], []
        for i in live:
            X = es[i].ask()
            ok = (np.ones(es[i].lam, dtype=bool) if feasibles[i] is None
                  else np.array([bool(feasibles[i](x)) for x in X]))
            Xs.append(X)
            oks.append(ok)
        fs = fun_many(list(live), [X[ok] for X, ok in zip(Xs, oks)])
        if len(fs) != len(live):
            raise ValueError(f"fun_many returned {len(fs)} value arrays for {len(live)} instances")
        for i, X, ok, fi in zip(live, Xs, oks, fs):
            f = np.full(es[i].lam, np.inf)
            if ok.any():
                f[ok] = np.asarray(fi, dtype=np.float64).ravel()
            es[i].tell(X, f)
        live = [i for i in live if es[i].stop() is None]
    return es


def _refine_steps(u0, feasible, max_iter):
    """refine_least_squares as a generator of requests: yields ("cost", u) and expects r(u).r(u) sent back, yields
    ("normal", u) and expects (J^T J, J^T r); returns the refined point."""
    u = np.array(u0, dtype=np.float64)
    c, mu = float((yield "cost", u)), 1e-3
    for _ in range(max_iter):
        G, g = yield "normal", u
        G, g = np.asarray(G, dtype=np.float64), np.asarray(g, dtype=np.float64)
        s = np.sqrt(np.diag(G))
        if not (np.all(np.isfinite(G)) and np.all(np.isfinite(g)) and np.all(s > 0)):
            break
        Gs, gs = G / np.outer(s, s), g / s
        while True:
            du = np.linalg.solve(Gs + mu * np.eye(u.size), -gs) / s
            un = u + du
            cn = float((yield "cost", un)) if (feasible is None or feasible(un)) else math.inf
            if cn < c:
                break
            mu *= 10.0
            if mu > 1e10:
                return u
        u, c, mu = un, cn, max(mu / 10.0, 1e-12)
        if np.abs(du).max() <= 1e-14 * max(1.0, np.abs(u).max()) or c == 0.0:
            break
    return u


def refine_least_squares(cost, normal, u0, feasible=None, max_iter=50):
    """Levenberg-Marquardt on a zero-residual least-squares problem, from u0: cost(u) = r(u).r(u), normal(u) =
    (J^T J, J^T r) at u.  A step is taken only when it lowers the cost, so the result is never worse than u0.  The
    estimator runs it on the best point of the CMA-ES: I(x) is a sum of norms whose minimum lies at the end of a long,
    curved, nearly flat valley (k / m is far less determined by the stored transitions than k l / m and m l^2), where
    the CMA-ES stopping rules fire long before the minimum; in the model's own constants the valley is straight and
    Gauss-Newton steps reach the minimum in a few iterations."""
    steps = _refine_steps(u0, feasible, max_iter)
    try:
        kind, u = next(steps)
        while True:
            kind, u = steps.send(cost(u) if kind == "cost" else normal(u))
    except StopIteration as done:
        return done.value


def refine_least_squares_many(cost_many, normal_many, U0, feasible=None, max_iter=50):
    """refine_least_squares for many independent problems in lock-step.  Every instance runs the same steps as the
    single function; per round all pending requests for normal equations are served by ONE call normal_many(idx, U)
    -> [(J^T J, J^T r) per entry] and all pending cost requests by ONE call cost_many(idx, U) -> [r.r per entry] (idx
    the instances' indices, U [len(idx), N] their points).  `feasible` is one rule for all or a list of one per
    instance.  Returns the list of refined points: instance i's iterates are those of refine_least_squares given the
    same callback values."""
    n = len(U0)
    feasible = list(feasible) if isinstance(feasible, (list, tuple)) else [feasible] * n
    steps = [_refine_steps(U0[i], feasible[i], max_iter) for i in range(n)]
    result, pending = [None] * n, {}

    def advance(i, value=None, first=False):
        try:
            pending[i] = next(steps[i]) if first else steps[i].send(value)
        except StopIteration as done:
            pending.pop(i, None)
            result[i] = done.value

    for i in range(n):
        advance(i, first=True)
    while pending:
        for kind, serve in (("normal", normal_many), ("cost", cost_many)):
            idx = [i for i in sorted(pending) if pending[i][0] == kind]
            if not idx:
                continue
            values = serve(idx, np.stack([pending[i][1] for i in idx]))
            if len(values) != len(idx):
                raise ValueError(f"{kind}_many returned {len(values)} values for {len(idx)} instances")
            for i, v in zip(idx, values):
                advance(i, v)
    return result


def to_constants(m_i, l_i, k):
    """(m_i, l_i, k) -> (k l / m, m l^2, k / m): the combinations the swimmer's step depends on (kl_m, c12 = 12 / (m
    l^2), six_k_m = 6 k / m; l = (k l / m) / (k / m))."""
    return np.array([k * l_i / m_i, m_i * l_i * l_i, k / m_i])


def from_constants(u):
    """The inverse of to_constants -> (m_i, l_i, k)."""
    l_i = u[0] / u[2]
    m_i = u[1] / (l_i * l_i)
    return np.array([m_i, l_i, u[2] * m_i])
