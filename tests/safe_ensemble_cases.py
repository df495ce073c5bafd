"""The case family of the ensemble safe-ARS tests: mixed_case of tests/test_safe_experiment_gpu.py -- three agents,
gated [1, 0, 1], policy 0.6 (2 rand - 1) and deltas from RandomState(1000 n + n_dir), nu = 0.4, the same threshold pairs
-- with an ensemble of E simulators around each of its three simulators: member 0 is the centre, member i the centre
+ 0.5 g / ||g||_2, g = RandomState(7 a + E).standard_normal(3) drawn in member order.  Host data only; the oracle's
answers are computed once per case and shared (never modified)."""
import functools

import numpy as np

import safe_ensemble_oracle as oracle_ens
from test_safe_experiment_gpu import COSTS, mixed_case

SPREAD = 0.5
# the two costs the oracle tests run: the reference's, and |thetadot_1|.  (|Gdot_x| and |Gdot_y| come within 1e-10 of
# their thresholds: the bit tests use them, a comparison with another arithmetic cannot)
CONDITIONED = (COSTS[0], COSTS[4])


def members(centre, a, E):
    """[E, 3] (l_i, m_i, k) around agent a's simulator."""
    rs = np.random.RandomState(7 * a + E)
    rows = [np.asarray(centre, dtype=np.float64)]
    for _ in range(1, E):
        g = rs.standard_normal(3)
        rows.append(rows[0] + SPREAD * g / np.linalg.norm(g))
    return np.array(rows)


def ensemble_case(n, n_dir, E, cost, flags=0):
    """mixed_case plus sims [3, E, 3]; c["sim"] stays the centres, which are the members 0."""
    c = mixed_case(n, n_dir, cost, flags)
    c["sims"] = np.stack([members(c["sim"][a], a, E) for a in range(3)])
    return c


@functools.lru_cache(maxsize=None)
def want(n, n_dir, E, k_cost, H):
    """The oracle's answers for ensemble_case(n, n_dir, E, CONDITIONED[k_cost]) over H steps."""
    return oracle_ens.batch(ensemble_case(n, n_dir, E, CONDITIONED[k_cost]), H)
