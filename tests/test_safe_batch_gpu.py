"""The safe batch on the GPU: the four kernels against their single-agent twins, SafeARSAgentBatch against independent
ARSAgent(safe=True) instances and against the reference's fixtures (tests/golden/safe_agent.npz), and the
safe_exploration sweep at a small size.  Everything but the fixtures is compared bit for bit."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:      # the quad-form child below runs this file as a script
    sys.path.insert(0, ROOT)

import swimmer_amd as sw  # noqa: E402
from swimmer_amd import kernels  # noqa: E402
from swimmer_amd._lib import SwParams  # noqa: E402
from swimmer_amd.ars import ars_agent, safe_exploration  # noqa: E402
from swimmer_amd.ars.parameters import Threshold  # noqa: E402

from batch_kernel_cases import SAFE_BATCH_FORMS, flags_of as _flags  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NU = 0.05
REAL = (0.8, 1.2, 10.2)
SIMS = [(0.81, 1.19, 10.1), (0.79, 1.21, 10.3), (0.8, 1.2, 10.2)]      # (l_i, m_i, k) per agent
F64 = dict(dtype=torch.float64, device=DEV)
I32 = dict(dtype=torch.int32, device=DEV)


def _inputs(n, N, S, v2):
    m, d = n - 1, 2 * n + 2
    rng = np.random.RandomState(1000 * n + 10 * N + S + (500 if v2 else 0))
    policy = torch.tensor(rng.uniform(-1, 1, (S, m, d)), device=DEV)
    deltas = torch.tensor(2 * rng.rand(S, N, m, d) - 1, device=DEV)
    mean = inv_std = None
    if v2:
        mean = torch.tensor(rng.uniform(-0.1, 0.1, (S, d)), device=DEV)
        inv_std = torch.tensor(rng.uniform(0.5, 2.0, (S, d)), device=DEV)
    return policy, deltas, mean, inv_std


def _row(t, a):
    return None if t is None else t[a]


def _np(t):
    return t.cpu().numpy()


def _check_gate(n, form, v2, S=3, N=9, H=40):
    """ars_gate_multi against one ars_gate call per agent in the agent's own simulator."""
    flags = _flags(form)
    base = SwParams.make(n, *REAL, 1e-3, (1.0, 0.0), flags=flags)
    policy, deltas, mean, inv_std = _inputs(n, N, S, v2)
    p_sim = [SwParams.make(n, *SIMS[a], 1e-3, (1.0, 0.0), flags=flags) for a in range(S)]
    # the agents' own simulator returns first (NaN threshold: everything admitted), to place the thresholds
    sim_ret = []
    for a in range(S):
        r = torch.empty(2 * N, **F64)
        kernels.ars_gate(p_sim[a], H, policy[a], deltas[a], NU, 0, N, np.nan, _row(mean, a), _row(inv_std, a),
                         returns=r)
        sim_ret.append(_np(r))
    assert not np.array_equal(sim_ret[0], sim_ret[1])          # different simulators, different policies
    # a threshold in the middle, one equal to a return (refuses that direction), one below everything
    # (the median of the per-direction minima: the directions at or below it are refused, the others admitted)
    thr = [float(np.median(np.minimum(sim_ret[0][0::2], sim_ret[0][1::2]))), float(sim_ret[1][2]), -np.inf]
    sim = torch.tensor(np.array(SIMS[:S]), device=DEV)
    returns = torch.full((S, 2 * N), np.nan, **F64)
    status = torch.full((S, 2 * N), -1, **I32)
    admit = torch.full((S, N), -1, **I32)
    out = kernels.ars_gate_multi(base, H, policy, deltas, NU, sim, torch.tensor(thr, **F64), mean, inv_std,
                                 returns=returns, status=status, admit=admit)
    assert out is admit
    for a in range(S):
        r1, s1 = torch.empty(2 * N, **F64), torch.full((2 * N,), -1, **I32)
        a1 = kernels.ars_gate(p_sim[a], H, policy[a], deltas[a], NU, 0, N, thr[a], _row(mean, a), _row(inv_std, a),
                              returns=r1, status=s1)
        assert np.array_equal(_np(returns[a]), _np(r1)), (a, "returns")
        assert np.array_equal(_np(status[a]), _np(s1)) and not _np(s1).any(), (a, "status")
        assert np.array_equal(_np(admit[a]), _np(a1)), (a, "admit")
    A = _np(admit)
    assert 0 < A[0].sum() < N and A[1][1] == 0 and A[2].all()
    return base, policy, deltas, mean, inv_std, admit, status


PATTERNS = [  # per round, per agent: hand-made admit flags over N = 9 directions
    ([0] * 9, [1] * 9, [1, 0, 1, 1, 0, 0, 1, 0, 0]),                    # k = 0, k = N, k = 4 scattered (one moment row)
    ([0, 1, 1, 0, 1, 1, 0, 1, 1], [0] * 9, [0, 0, 0, 0, 0, 1, 1, 1, 1]),  # k = 6, k = 0, k = 4 at the end
]


def _check_counted(n, form, v2, S=3, N=9, H=40):
    """ars_pack_admitted, ars_rollouts_multi_counted and ars_update_multi_counted on hand-made flags against
    ars_rollouts / ars_update with n_dir = k on the packed deltas."""
    p = SwParams.make(n, *REAL, 1e-3, (1.0, 0.0), flags=_flags(form))
    m, d = p.m, p.d
    policy0, deltas, mean0, inv_std0 = _inputs(n, N, S, v2)
    rows = kernels.moments_blocks(2 * N)
    assert rows == 2
    running0 = torch.zeros((S, 1 + 2 * d), **F64) if v2 else None
    if v2 and form == "twin":
        # The twin barely moves in 40 steps from its 0.001 start (Gdot x: a spread of 5e-7), and statistics made of
        # such a round alone whiten the next one into a feedback gain of 2e6: the simulator itself diverges to NaN
        # within 30 steps (on the CPU oracle too), and NaN returns compare unequal.  So the twin's agents start, as
        # an agent does after an iteration, from running statistics that already hold 2 N H states of unit variance.
        running0[:, 0] = 2 * N * H
        running0[:, 1 + d:] = 2 * N * H
    state = dict(policy=policy0.clone(), running=running0,
                 mean=mean0, inv_std=inv_std0, sigma=torch.zeros(S, **F64))
    alpha, b = 0.02, float(N)
    seen = set()
    for flags in PATTERNS:
        admit = torch.tensor(np.array(flags), **I32)
        packed = torch.full((S, N, m, d), 7.0, **F64)
        count, order, out = kernels.ars_pack_admitted(p, admit, deltas, packed=packed)
        assert out is packed
        C, O, P = _np(count), _np(order), _np(packed)
        for a in range(S):
            idx = np.flatnonzero(flags[a])
            k = len(idx)
            seen.add(k)
            assert C[a] == k
            assert np.array_equal(O[a, :k], idx) and (O[a, k:] == -1).all()
            assert np.array_equal(P[a, :k], _np(deltas[a])[idx]) and (P[a, k:] == 7.0).all()
        # ---- the counted rollouts: entries 0 .. 2k - 1 and the first ceil(2k / 16) moment rows, nothing else
        returns = torch.full((S, 2 * N), 5.0, **F64)
        status = torch.full((S, 2 * N), -1, **I32)
        moments = torch.full((S, rows, 2 * d), 9.0, **F64) if v2 else None
        kernels.ars_rollouts_multi_counted(p, H, state["policy"], packed, NU, count, state["mean"], state["inv_std"],
                                           returns=returns, moments=moments, status=status)
        R, St = _np(returns), _np(status)
        single_moments = []
        for a in range(S):
            k = int(C[a])
            rk = kernels.moments_blocks(2 * k)
            assert (R[a, 2 * k:] == 5.0).all() and (St[a, 2 * k:] == -1).all()
            if v2:
                assert (_np(moments[a, rk:]) == 9.0).all()
            single_moments.append(None)
            if k == 0:
                continue
            m1 = torch.zeros((rk, 2 * d), **F64) if v2 else None
            s1 = torch.full((2 * k,), -1, **I32)
            r1 = kernels.ars_rollouts(p, H, state["policy"][a], packed[a], NU, 0, k, _row(state["mean"], a),
                                      _row(state["inv_std"], a), moments=m1, status=s1)
            assert np.array_equal(R[a, :2 * k], _np(r1)), (a, "returns")
            assert not St[a, :2 * k].any() and not _np(s1).any()
            if v2:
                assert np.array_equal(_np(moments[a, :rk]), _np(m1)), (a, "moment rows")
            single_moments[a] = m1
        # ---- the counted update against ars_update with n_dir = k, from the same state, top_b 0 and 2
        for top_b in (0, 2):
            multi = {k_: None if v is None else v.clone() for k_, v in state.items()}
            kernels.ars_update_multi_counted(p, H, count, returns, packed, multi["policy"], alpha, b, top_b,
                                             moments=moments, running=multi["running"], mean=multi["mean"],
                                             inv_std=multi["inv_std"], sigma_out=multi["sigma"])
            for a in range(S):
                k = int(C[a])
                one = {k_: None if v is None else v[a].clone() for k_, v in state.items()}
                one["sigma"] = state["sigma"][a:a + 1].clone()
                if k > 0:
                    kernels.ars_update(p, returns[a, :2 * k].contiguous(), packed[a, :k].contiguous(), one["policy"],
                                       alpha, b, top_b, moments=single_moments[a], running=one["running"],
                                       n_new_states=2 * k * H, mean=one["mean"] if v2 else None,
                                       inv_std=one["inv_std"] if v2 else None, sigma_out=one["sigma"])
                # k = 0: `one` is the state before the call, which the batch must have left untouched
                names = ("policy", "sigma") + (("running", "mean", "inv_std") if v2 else ())
                for name in names:
                    got = multi[name][a:a + 1] if name == "sigma" else multi[name][a]
                    assert np.array_equal(_np(got), _np(one[name])), (top_b, a, k, name)
                if k > 0:
                    assert not np.array_equal(_np(multi["policy"][a]), _np(state["policy"][a]))
            state = multi          # the next round starts from non-zero running statistics (top_b = 2's result)
    assert seen == {0, 4, 6, N}
    # a direction whose gate status is non-zero on either rollout is packed out
    admit = torch.ones((S, N), **I32)
    gate_status = torch.zeros((S, 2 * N), **I32)
    gate_status[0, 2 * 3] = 1           # agent 0, direction 3, + rollout
    gate_status[2, 2 * 8 + 1] = 2       # agent 2, direction 8, - rollout
    count, order, _ = kernels.ars_pack_admitted(p, admit, deltas, status=gate_status)
    assert _np(count).tolist() == [N - 1, N, N - 1]
    assert _np(order[0]).tolist() == [0, 1, 2, 4, 5, 6, 7, 8, -1]
    assert _np(order[2]).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, -1]


def _check_form(n, form):
    for v2 in (False, True):
        _check_gate(n, form, v2)
        _check_counted(n, form, v2)


@pytest.mark.parametrize("n,form", [c[:2] for c in SAFE_BATCH_FORMS], ids=[c[2] for c in SAFE_BATCH_FORMS])
def test_kernels_equal_their_single_agent_twins(n, form):
    """SAFE_BATCH_FORMS (tests/batch_kernel_cases.py): mirror-quad, the row form at every n = 4..8, the lane form at
    every n = 2..8 in both models ("twin": the agents' (l_i, m_i, k) are the twin's constants as they are)."""
    _check_form(n, form)


def test_kernels_in_the_quad_form_in_a_child_process():
    """SWIMMER_N3_KERNEL=quad (read once per process) sends n = 3 to the quad form: batch and single launches alike."""
    env = dict(os.environ, SWIMMER_N3_KERNEL="quad")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "quad-child"], env=env, capture_output=True,
                          text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "quad-child ok" in done.stdout


def test_gate_marks_a_simulator_that_breaks_the_parameter_rule():
    n, S, N, H = 3, 3, 9, 40
    base = SwParams.make(n, *REAL, 1e-3, (1.0, 0.0))
    policy, deltas, _, _ = _inputs(n, N, S, False)
    thr = torch.full((S,), -np.inf, **F64)
    good = torch.tensor(np.array(SIMS), device=DEV)
    bad = good.clone()
    bad[1, 0] = -1.0                    # l_i < 0
    ret_g, st_g = torch.zeros((S, 2 * N), **F64), torch.zeros((S, 2 * N), **I32)
    ret_b, st_b = torch.zeros((S, 2 * N), **F64), torch.zeros((S, 2 * N), **I32)
    adm_g = kernels.ars_gate_multi(base, H, policy, deltas, NU, good, thr, returns=ret_g, status=st_g)
    adm_b = kernels.ars_gate_multi(base, H, policy, deltas, NU, bad, thr, returns=ret_b, status=st_b)
    assert _np(adm_g).all()
    assert (_np(st_b[1]) == 8).all() and not _np(adm_b[1]).any() and np.isnan(_np(ret_b[1])).all()   # SW_STATUS_PARAM
    for a in (0, 2):
        assert np.array_equal(_np(ret_b[a]), _np(ret_g[a])) and not _np(st_b[a]).any() and _np(adm_b[a]).all()


# ---- the batch against independent safe agents ------------------------------------------------------------------
def _real(n, H):
    return sw.EnvParam("RealWorld", n=n, H=H, l_i=0.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0.001)


@pytest.mark.parametrize("n,V1,N", [(3, True, 1), (3, False, 9), (6, False, 4)], ids=["n3-V1-N1", "n3-V2-N9", "n6-V2-N4"])
def test_batch_equals_independent_safe_agents(n, V1, N, tmp_path):
    from test_safe_ars_agent_cpu import DB
    S, H, iters = 3, 60, 4
    m, d = n - 1, 2 * n + 2
    w0 = str(tmp_path / "w0.npy")
    np.save(w0, np.random.RandomState(7).uniform(-1, 1, (m, d)))
    ep = _real(n, H)
    ap = sw.ARSParam("S", V1=V1, n_iter=iters - 1, H=H, N=N, b=N, alpha=0.0075, nu=0.1, safe=True, threshold=0.0,
                     initial_w=w0)
    agents = []
    for s in range(S):
        np.random.seed(100 + s)
        agents.append(sw.ARSAgent(copy.copy(ep), ap, data_path=DB, seed=s, approx_error=1e-3,
                                  sim_thresh=Threshold(1, 0.3, 0.001), full_covariance=False))
    assert ep.l_i == 0.8 and len({a.estimated_param.l_i for a in agents}) == S
    # agent 0 always admitted, agent 1 always refused, agent 2 in the middle of its first iteration's simulator returns
    np.random.seed(2)
    first = 2 * np.random.rand(N, m, d) - 1
    sims = _np(kernels.ars_rollouts(agents[2].p_sim, H, torch.tensor(agents[2].policy, device=DEV),
                                    torch.tensor(first, device=DEV), ap.nu, 0, N, mean=agents[2]._mean,
                                    inv_std=agents[2]._inv_std))
    sim_thr = [-1e9, 1e9, float(np.median(np.minimum(sims[0::2], sims[1::2])) + 1e-9)]
    # the single agents share NumPy's global generator: one after the other, each from its own seed
    record = []
    for s, agent in enumerate(agents):
        agent.sim_threshold = sim_thr[s]
        np.random.seed(s)
        rows = []
        for _ in range(iters):
            r = agent.runOneIteration()
            rows.append((r, agent.last_admitted.copy(), agent.policy, agent.mean))
        record.append(rows)
    batch = sw.SafeARSAgentBatch(ep, ap, range(S), [a.estimated_param for a in agents], sim_thr)
    ks = set()
    for it in range(iters):
        rets = batch.runOneIteration()
        pol, mean = batch.policy, batch.mean
        for s in range(S):
            r, admitted, p1, m1 = record[s][it]
            assert np.array_equal(rets[s], r), (it, s, "returns")
            assert np.array_equal(batch.last_admitted[s], admitted), (it, s, "admitted")
            assert np.array_equal(pol[s], p1), (it, s, "policy")
            if not V1:
                assert np.array_equal(mean[s], m1), (it, s, "mean")
            ks.add(len(admitted))
    assert np.array_equal(batch.violations, [a.violations for a in agents])
    assert 0 in ks and N in ks
    if N >= 2:
        assert any(0 < k < N for k in ks)
        assert 0 < len(record[2][0][1]) < N          # by construction: agent 2's first iteration


# ---- the reference's own fixtures -------------------------------------------------------------------------------
def _golden_batch(tags, fillers, tmp_path):
    """One SafeARSAgentBatch holding the golden cases `tags` as agents 0.. and `fillers` more agents behind them."""
    from test_safe_ars_agent_cpu import _fixture, _params
    g = _fixture()
    cases = [_params(g, t) for t in tags]
    ep, ap = cases[0][0], cases[0][1]
    for ep_, ap_, _, c_ in cases[1:]:        # what a batch shares
        assert (ep_.n, ep_.H, ep_.l_i, ep_.m_i, ep_.k, ep_.h) == (ep.n, ep.H, ep.l_i, ep.m_i, ep.k, ep.h)
        assert (ap_.V1, ap_.n_iter, ap_.H, ap_.N, ap_.b, ap_.alpha, ap_.nu) == \
               (ap.V1, ap.n_iter, ap.H, ap.N, ap.b, ap.alpha, ap.nu)
    sims, seeds, sim_thr, thr, w0 = [], [], [], [], []
    for t, (ep_, ap_, _, c_) in zip(tags, cases):
        l_i, m_i, k, h = g[t + "_estimated"]
        sims.append(sw.EnvParam("LeonSwimmer-Simulator", n=ep.n, H=ep.H, l_i=l_i, m_i=m_i, h=h, k=k,
                                epsilon=ep_.epsilon))
        seeds.append(c_["seed"])
        sim_thr.append(float(g[t + "_sim_threshold"]))
        thr.append(ap_.threshold)
        w0.append(g[t + "_w0"])
    for f in range(fillers):                 # always admitted, another stream
        sims.append(copy.copy(sims[0]))
        seeds.append(seeds[0] + 1 + f)
        sim_thr.append(-1e9)
        thr.append(thr[0])
        w0.append(w0[0])
    batch = sw.SafeARSAgentBatch(ep, ap, seeds, sims, sim_thr, thresholds=thr)
    batch.policy = np.stack(w0)
    return g, batch, ap


@pytest.mark.parametrize("tags,fillers", [("ah", 1), ("ef", 0), ("b", 2)], ids=["a+h", "e+f", "b"])
def test_batch_matches_the_reference(tags, fillers, tmp_path):
    from test_safe_ars_agent_cpu import _close
    g, batch, ap = _golden_batch(tags, fillers, tmp_path)
    per_it, inner = [], batch._read

    def recorded(rows):
        out = inner(rows)
        per_it.extend(out)
        return out
    batch._read = recorded
    curves = batch.runTraining()
    assert len(per_it) == ap.n_iter + 1
    policy, mean = batch.policy, batch.mean
    for s, tag in enumerate(tags):
        counts = np.array([len(r[s]) for r in per_it])
        assert np.array_equal(counts, g[tag + "_counts"])          # admitted / refused pattern
        for j, r in enumerate(per_it):
            _close(r[s], g[tag + "_returns"][j][:len(r[s])])
        _close(curves[s], g[tag + "_curve"])                       # NaN warm-up of a refused first iteration included
        _close(policy[s], g[tag + "_policy"])
        if not ap.V1:
            _close(mean[s], g[tag + "_mean"])
        assert batch.violations[s] == int(g[tag + "_below"])
    if tags == "ef":
        ks = {tuple(np.unique(g[t + "_counts"])) for t in tags}
        assert ks == {(0,), (2 * ap.N,)}                           # one admits everything, the other nothing


# ---- the sweep -------------------------------------------------------------------------------------------------
def test_safe_exploration_run_at_a_small_size(tmp_path):
    A_values, eps, n_seed, H = (0.1, 0.5), (0.001, 0.01), 2, 50
    results, data = str(tmp_path / "results"), str(tmp_path / "data")
    out = safe_exploration.run(A_values=A_values, epsilons=eps, n_seed=n_seed, n_iter=3, hand_iter=3, H=H,
                               results_path=results, data_path=data, rng=np.random.RandomState(5))
    assert out["r_graphs"].shape == (2, 2, n_seed, 4)
    for name in ("min_return", "max_mean_returns", "sim_thresh_range"):
        assert len(out[name]) == 2 and all(np.shape(x) == (2,) for x in out[name])
    l = out["l"]
    assert float(np.loadtxt(os.path.join(data, "threshold.txt"))) == pytest.approx(l, rel=1e-15)
    hand = np.load(os.path.join(data, "saved_hand_policy.npy"))
    assert hand.shape == (2, 8)
    for i, A in enumerate(A_values):
        alpha = Threshold(K=1, A=A, B=0.001).compute_alpha(H)
        assert np.array_equal(out["sim_thresh_range"][i], [l + alpha * e for e in eps])
        try:
            import matplotlib  # noqa: F401
        except ImportError:
            continue
        assert os.path.exists(os.path.join(results, f"epsilon_sim_threshold_H={H}_K=1_A={A}_B=0.001.png"))
    # the same agents built by hand from the same draws
    rng = np.random.RandomState(5)
    seeds, sims, thr = [], [], []
    for A in A_values:
        alpha = Threshold(K=1, A=A, B=0.001).compute_alpha(H)
        for e in eps:
            real = sw.EnvParam('LeonSwimmer-RealWorld', n=3, H=H, l_i=.8, m_i=1.2, h=1e-3, k=10.2, epsilon=e)
            sims += ars_agent.approximate_env_params(real, e, n_seed, rng)
            seeds += list(range(n_seed))
            thr += [l + alpha * e] * n_seed
    ap = sw.ARSParam('RLControl', V1=True, n_iter=3, H=H, N=1, b=1, alpha=0.0075, nu=0.01, safe=True, threshold=l,
                     initial_w=os.path.join(data, "saved_hand_policy.npy"))
    curves = sw.SafeARSAgentBatch(safe_exploration.real_world(H), ap, seeds, sims, thr).runTraining()
    assert np.array_equal(curves.reshape(out["r_graphs"].shape), out["r_graphs"], equal_nan=True)
    g = out["r_graphs"]
    for i in range(2):
        assert np.array_equal(out["min_return"][i], [np.nanmin(g[i, j]) for j in range(2)], equal_nan=True)


def test_a_failed_simulator_rollout_names_its_agent_and_spares_the_others(tmp_path):
    n, H, N, S = 3, 50, 4, 3
    ep = _real(n, H)
    w0 = str(tmp_path / "w0.npy")
    np.save(w0, np.random.RandomState(7).uniform(-1, 1, (2, 8)))
    ap = sw.ARSParam("S", V1=False, n_iter=1, H=H, N=N, b=N, alpha=0.0075, nu=0.1, safe=True, threshold=0.0,
                     initial_w=w0)
    sims = ars_agent.approximate_env_params(ep, 1e-3, S, np.random.RandomState(3))

    def make():
        return sw.SafeARSAgentBatch(ep, ap, [4, 5, 6], sims, [-1e9] * S)
    healthy, broken = make(), make()
    P = broken.policy
    P[1] = 1e300                         # agent 1's simulator state blows up at once
    broken.policy = P
    good = healthy.runOneIteration()
    with pytest.raises(np.linalg.LinAlgError) as err:
        broken.runOneIteration()
    text = str(err.value)
    assert "seed 5" in text and "seed 4" not in text and "seed 6" not in text
    assert len(broken.last_returns[1]) == 0 and len(broken.last_admitted[1]) == 0      # nothing unsafe ran
    assert np.array_equal(broken.policy[1], P[1])
    for s in (0, 2):
        assert np.array_equal(broken.last_returns[s], good[s]) and len(good[s]) == 2 * N
        assert np.array_equal(broken.last_admitted[s], healthy.last_admitted[s])
        assert np.array_equal(broken.policy[s], healthy.policy[s])
        assert np.array_equal(broken.mean[s], healthy.mean[s])


if __name__ == "__main__" and sys.argv[1:] == ["quad-child"]:
    # the child of test_kernels_in_the_quad_form_in_a_child_process
    _check_form(3, "auto")
    print("quad-child ok")
