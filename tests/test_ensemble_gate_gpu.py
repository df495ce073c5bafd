"""The ensemble gate on the GPU: every member of sw_ars_gate_ensemble_f64 against the single gate in that member's
simulator, the fold against its NumPy restatement (ars/ensemble.py), E = 1 against the multi-agent gate, the member
returns against the CPU oracle, and ARSAgent / SafeARSAgentBatch / run_ensemble gating with an ensemble.  Everything
but the oracle comparison is bit for bit."""
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
from swimmer_amd._lib import STATUS_PARAM, SwParams  # noqa: E402
from swimmer_amd.ars import ars_agent, safe_exploration  # noqa: E402
from swimmer_amd.ars.ensemble import fold_reference, sphere_ensemble  # noqa: E402
from swimmer_amd.ars.ensemble_kernels import ars_gate_ensemble  # noqa: E402
from swimmer_amd.ars.parameters import Threshold  # noqa: E402

from batch_kernel_cases import ENSEMBLE_FORMS as FORMS, flags_of as _flags  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NU = 0.05
REAL = (0.8, 1.2, 10.2)
# (l_i, m_i, k) of member e of agent a: distinct within and across the agents, one of them the real world
SIMS = [[(0.81, 1.19, 10.1), (0.79, 1.21, 10.3), (0.8, 1.2, 10.2)],
        [(0.82, 1.18, 10.0), (0.78, 1.22, 10.4), (0.805, 1.195, 10.15)],
        [(0.83, 1.17, 9.9), (0.77, 1.23, 10.5), (0.795, 1.205, 10.25)]]
F64 = dict(dtype=torch.float64, device=DEV)
I32 = dict(dtype=torch.int32, device=DEV)
GUARD = 64


def _np(t):
    return t.cpu().numpy()


def _row(t, a):
    return None if t is None else t[a]


def _inputs(n, N, S, v2):
    m, d = n - 1, 2 * n + 2
    rng = np.random.RandomState(2000 * n + 10 * N + S + (500 if v2 else 0))
    policy = torch.tensor(rng.uniform(-1, 1, (S, m, d)), device=DEV)
    deltas = torch.tensor(2 * rng.rand(S, N, m, d) - 1, device=DEV)
    mean = inv_std = None
    if v2:
        mean = torch.tensor(rng.uniform(-0.1, 0.1, (S, d)), device=DEV)
        inv_std = torch.tensor(rng.uniform(0.5, 2.0, (S, d)), device=DEV)
    return policy, deltas, mean, inv_std


def _guarded(shape, fill, **kw):
    """A tensor of `shape` filled with a sentinel in the middle of a larger buffer of it: (buffer, view)."""
    size = int(np.prod(shape))
    buf = torch.full((size + 2 * GUARD,), fill, **kw)
    return buf, buf[GUARD:GUARD + size].view(shape)


def _intact(buf, fill):
    b = _np(buf)
    edge = np.concatenate([b[:GUARD], b[-GUARD:]])
    return bool(np.isnan(edge).all()) if isinstance(fill, float) and np.isnan(fill) else bool((edge == fill).all())


def _single_gates(p_sim, H, policy, deltas, mean, inv_std, thr):
    """kernels.ars_gate per (agent, member) -> returns, status [S][E][2N] and flags [S][E][N] as NumPy arrays."""
    S, E, N = len(p_sim), len(p_sim[0]), deltas.shape[1]
    R, St, A = np.empty((S, E, 2 * N)), np.empty((S, E, 2 * N), np.int32), np.empty((S, E, N), np.int32)
    for a in range(S):
        for e in range(E):
            r, s = torch.empty(2 * N, **F64), torch.full((2 * N,), -1, **I32)
            adm = kernels.ars_gate(p_sim[a][e], H, policy[a], deltas[a], NU, 0, N, thr[a], _row(mean, a),
                                   _row(inv_std, a), returns=r, status=s)
            R[a, e], St[a, e], A[a, e] = _np(r), _np(s), _np(adm)
    return R, St, A


def _check_members_and_fold(n, form, v2, N=9, S=3, E=3, H=40):
    flags = _flags(form)
    base = SwParams.make(n, *REAL, 1e-3, (1.0, 0.0), flags=flags)
    p_sim = [[SwParams.make(n, *SIMS[a][e], 1e-3, (1.0, 0.0), flags=flags) for e in range(E)] for a in range(S)]
    assert REAL in SIMS[0] and len({s for row in SIMS for s in row}) == S * E
    policy, deltas, mean, inv_std = _inputs(n, N, S, v2)
    # the single gates first, under a NaN threshold (everything admitted), to place the thresholds
    R0, St0, _ = _single_gates(p_sim, H, policy, deltas, mean, inv_std, [np.nan] * S)
    assert not St0.any() and np.isfinite(R0).all()
    assert len({R0[a, e].tobytes() for a in range(S) for e in range(E)}) == S * E      # the simulators differ
    worst0 = R0.min(axis=1)                                                            # [S][2N]
    # agent 0: in the middle of its WORST returns; agent 1: equal to one member's return of direction 1; agent 2: open
    thr = [float(np.median(np.minimum(worst0[0][0::2], worst0[0][1::2]))), float(R0[1, 1, 2]), -np.inf]
    R1, St1, A1 = _single_gates(p_sim, H, policy, deltas, mean, inv_std, thr)
    assert np.array_equal(R1, R0)
    all_admit = A1.all(axis=1)
    assert 0 < all_admit[0].sum() < N                       # conditions on the inputs, from the single gates
    assert A1[1, 1, 1] == 0 and all_admit[1, 1] == 0        # equality refuses that direction
    assert all_admit[2].all()
    sim = torch.tensor(np.array(SIMS)[:S, :E], device=DEV)
    bufs = dict(admit=_guarded((S, N), -7, **I32), worst=_guarded((S, 2 * N), np.nan, **F64),
                status=_guarded((S, 2 * N), -7, **I32), member_returns=_guarded((S, E, 2 * N), np.nan, **F64),
                member_status=_guarded((S, E, 2 * N), -7, **I32), member_admit=_guarded((S, E, N), -7, **I32))
    out = ars_gate_ensemble(base, H, policy, deltas, NU, sim, torch.tensor(thr, **F64), mean, inv_std,
                            **{k: v[1] for k, v in bufs.items()})
    assert out[0] is bufs["admit"][1] and out[1] is bufs["worst"][1]
    got = {k: _np(v[1]) for k, v in bufs.items()}
    for a in range(S):
        for e in range(E):
            assert np.array_equal(got["member_returns"][a, e], R1[a, e]), (a, e, "returns")
            assert np.array_equal(got["member_status"][a, e], St1[a, e]), (a, e, "status")
            assert np.array_equal(got["member_admit"][a, e], A1[a, e]), (a, e, "admit")
    # the fold: the restatement on the member arrays, exactly; the invariant; nothing written outside the outputs
    m_adm, admit, worst, status = fold_reference(got["member_returns"], got["member_status"], np.array(thr))
    assert np.array_equal(got["member_admit"], m_adm)
    assert np.array_equal(got["admit"], admit) and got["admit"].dtype == np.int32
    assert np.array_equal(got["worst"], worst) and np.array_equal(worst, worst0)
    assert np.array_equal(got["status"], status) and not status.any()
    t = np.array(thr)[:, None]
    assert np.array_equal(got["admit"].astype(bool), ~(worst[:, 0::2] <= t) & ~(worst[:, 1::2] <= t))
    for name, (buf, _) in bufs.items():
        assert _intact(buf, np.nan if buf.dtype == torch.float64 else -7), name
    # the optional status may be left out, and the member arrays are allocated when not given
    a2, w2 = ars_gate_ensemble(base, H, policy, deltas, NU, sim, torch.tensor(thr, **F64), mean, inv_std)
    assert np.array_equal(_np(a2), got["admit"]) and np.array_equal(_np(w2), got["worst"])
    return base, policy, deltas, mean, inv_std, got


def _check_one_member_equals_the_multi_gate(n, form, v2, N=9, S=3, H=40):
    base = SwParams.make(n, *REAL, 1e-3, (1.0, 0.0), flags=_flags(form))
    policy, deltas, mean, inv_std = _inputs(n, N, S, v2)
    sim = torch.tensor(np.array([SIMS[a][a] for a in range(S)]), device=DEV)              # [S, 3]
    open_ret = torch.empty((S, 2 * N), **F64)
    kernels.ars_gate_multi(base, H, policy, deltas, NU, sim, torch.full((S,), np.nan, **F64), mean, inv_std,
                           returns=open_ret)
    r = _np(open_ret)
    thr = torch.tensor([float(np.median(np.minimum(r[0, 0::2], r[0, 1::2]))), float(r[1, 3]), -np.inf], **F64)
    ret, st = torch.empty((S, 2 * N), **F64), torch.full((S, 2 * N), -1, **I32)
    adm = kernels.ars_gate_multi(base, H, policy, deltas, NU, sim, thr, mean, inv_std, returns=ret, status=st)
    status = torch.full((S, 2 * N), -1, **I32)
    m_ret, m_st = torch.empty((S, 1, 2 * N), **F64), torch.full((S, 1, 2 * N), -1, **I32)
    m_adm = torch.full((S, 1, N), -1, **I32)
    admit, worst = ars_gate_ensemble(base, H, policy, deltas, NU, sim[:, None, :].contiguous(), thr, mean, inv_std,
                                     status=status, member_returns=m_ret, member_status=m_st, member_admit=m_adm)
    assert 0 < _np(adm)[0].sum() < N and _np(adm)[1, 1] == 0 and _np(adm)[2].all()
    assert np.array_equal(_np(admit), _np(adm)) and np.array_equal(_np(m_adm[:, 0]), _np(adm))
    assert np.array_equal(_np(worst), _np(ret)) and np.array_equal(_np(m_ret[:, 0]), _np(ret))
    assert np.array_equal(_np(status), _np(st)) and np.array_equal(_np(m_st[:, 0]), _np(st))


def _check_form(n, form, N=9):
    for v2 in (False, True):
        _check_members_and_fold(n, form, v2, N=N)
        _check_one_member_equals_the_multi_gate(n, form, v2, N=N)


@pytest.mark.parametrize("n,form,N", FORMS, ids=[f"n{n}-{form}-N{N}" for n, form, N in FORMS])
def test_members_equal_the_single_gate_and_the_fold_its_restatement(n, form, N):
    """ENSEMBLE_FORMS (tests/batch_kernel_cases.py).  n = 3 auto: mirror-quad; n = 4..8 auto: row; n = 2 and 'lane' /
    'twin': one rollout per lane, every n = 2..8 in both models (N = 33: 66 rollouts cross its 64-slot workgroup);
    2N = 18 crosses the 16-slot group of the other forms."""
    _check_form(n, form, N)


def test_the_quad_form_in_a_child_process():
    """SWIMMER_N3_KERNEL=quad (read once per process) sends n = 3 to the quad form: ensemble and single launches."""
    env = dict(os.environ, SWIMMER_N3_KERNEL="quad")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "quad-child"], env=env, capture_output=True,
                          text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "quad-child ok" in done.stdout


@pytest.mark.parametrize("n,form", [(3, "auto"), (6, "auto"), (3, "lane")], ids=["mirror-quad", "row", "lane"])
def test_a_member_that_breaks_the_parameter_rule_silences_its_agent_only(n, form):
    S, E, N, H = 3, 3, 9, 40
    base = SwParams.make(n, *REAL, 1e-3, (1.0, 0.0), flags=_flags(form))
    policy, deltas, _, _ = _inputs(n, N, S, False)
    thr = torch.full((S,), -np.inf, **F64)
    good = torch.tensor(np.array(SIMS), device=DEV)
    bad = good.clone()
    bad[1, 2, 1] = -1.0                                   # agent 1, member 2: m_i = -1

    def run(sim):
        out = dict(status=torch.full((S, 2 * N), -1, **I32), member_returns=torch.zeros((S, E, 2 * N), **F64),
                   member_status=torch.full((S, E, 2 * N), -1, **I32), member_admit=torch.full((S, E, N), -1, **I32))
        admit, worst = ars_gate_ensemble(base, H, policy, deltas, NU, sim, thr, **out)
        return dict({k: _np(v) for k, v in out.items()}, admit=_np(admit), worst=_np(worst))
    g, b = run(good), run(bad)
    assert g["admit"].all() and not g["status"].any()
    assert (b["member_status"][1, 2] == STATUS_PARAM).all() and np.isnan(b["member_returns"][1, 2]).all()
    assert not b["member_admit"][1, 2].any() and not b["admit"][1].any()
    assert (b["status"][1] == STATUS_PARAM).all()
    for e in (0, 1):                                      # the agent's other members ran as before
        for name in ("member_returns", "member_status", "member_admit"):
            assert np.array_equal(b[name][1, e], g[name][1, e])
    assert np.array_equal(b["worst"][1], g["member_returns"][1, :2].min(axis=0))
    for a in (0, 2):
        for name in g:
            assert np.array_equal(b[name][a], g[name][a]), (a, name)


def test_a_pessimistic_member_refuses_what_the_real_world_alone_admits():
    n, N, H = 3, 9, 40
    base = SwParams.make(n, *REAL, 1e-3, (1.0, 0.0))
    policy, deltas, _, _ = _inputs(n, N, 1, False)
    pessimist = (0.8, 1.2, 14.0)                          # a much more viscous world: other returns
    p = [SwParams.make(n, *REAL, 1e-3, (1.0, 0.0)), SwParams.make(n, *pessimist, 1e-3, (1.0, 0.0))]
    R, _, _ = _single_gates([p], H, policy, deltas, None, None, [np.nan])
    lo_real, lo_pess = (np.minimum(R[0, e, 0::2], R[0, e, 1::2]) for e in (0, 1))
    # the direction the pessimist thinks worst of, next to the real world's opinion: a threshold between the two
    # members' returns of it admits it in the real world alone and refuses it in the ensemble
    j = int(np.argmax(lo_real - lo_pess))
    assert lo_pess[j] < lo_real[j]                       # a condition on the inputs, from the single gates
    thr = torch.tensor([0.5 * (lo_pess[j] + lo_real[j])], **F64)
    one = torch.tensor(np.array([[REAL]]), device=DEV)
    two = torch.tensor(np.array([[REAL, pessimist]]), device=DEV)
    a1, w1 = ars_gate_ensemble(base, H, policy, deltas, NU, one, thr)
    a2, w2 = ars_gate_ensemble(base, H, policy, deltas, NU, two, thr)
    assert _np(a1)[0, j] == 1 and _np(a2)[0, j] == 0 and _np(a2)[0].sum() < _np(a1)[0].sum()
    assert np.array_equal(_np(w1)[0], R[0, 0]) and np.array_equal(_np(w2)[0], R[0].min(axis=0))


@pytest.mark.parametrize("n", [3, 6])
def test_member_returns_against_the_oracle(n):
    """The tolerance tests/test_safe_ars_agent_gpu.py holds sw_ars_gate_f64 to: 1e-12 relative to max(1, |ref|)."""
    from oracle import swimmer_oracle as so
    from conftest import observed
    S, E, N, H = 2, 3, 5, 40
    m, d = n - 1, 2 * n + 2
    base = SwParams.make(n, *REAL, 1e-3, (1.0, 0.0))
    policy, deltas, _, _ = _inputs(n, N, S, False)
    sim = torch.tensor(np.array(SIMS)[:S, :E], device=DEV)
    m_ret = torch.empty((S, E, 2 * N), **F64)
    ars_gate_ensemble(base, H, policy, deltas, NU, sim, torch.full((S,), -np.inf, **F64), member_returns=m_ret)
    got, P, D = _np(m_ret), _np(policy), _np(deltas)
    worst = 0.0
    for a in range(S):
        pols = np.empty((2 * N, m, d))
        pols[0::2], pols[1::2] = P[a] + NU * D[a], P[a] - NU * D[a]
        for e in range(E):
            ref, _ = so.rollout_batch(so.OracleParams.make(n, *SIMS[a][e], 1e-3), H, pols)
            err = np.abs(got[a, e] - ref) / np.maximum(1.0, np.abs(ref))
            worst = max(worst, float(err.max()))
    observed(f"ensemble_gate_member_returns_n{n}", {"max_rel_err": worst, "tolerance": 1e-12, "H": H, "N": N})
    assert worst <= 1e-12, worst


# ---- the agents -------------------------------------------------------------------------------------------------
def _real(n, H):
    return sw.EnvParam("RealWorld", n=n, H=H, l_i=0.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0.001)


def _ensemble(ep, a, E=3):
    out = []
    for e in range(E):
        s = copy.copy(ep)
        s.l_i, s.m_i, s.k = SIMS[a][e]
        out.append(s)
    return out


def _agent_param(N, H, w0, iters=3, V1=False, threshold=0.0):
    return sw.ARSParam("S", V1=V1, n_iter=iters, H=H, N=N, b=N, alpha=0.0075, nu=0.1, safe=True, threshold=threshold,
                       initial_w=w0)


def _first_worst(agent, ap, ensemble, seed):
    """The worst of the single gates over `ensemble` for the deltas the agent draws first after np.random.seed(seed)."""
    np.random.seed(seed)
    first = torch.tensor(2 * np.random.rand(ap.N, agent.m, agent.d) - 1, device=DEV)
    rows = []
    for sp in ensemble:
        p = SwParams.make(sp.n, sp.l_i, sp.m_i, sp.k, sp.h, (1.0, 0.0))
        r = torch.empty(2 * ap.N, **F64)
        kernels.ars_gate(p, ap.H, agent._policy, first, ap.nu, 0, ap.N, np.nan, agent._mean, agent._inv_std, returns=r)
        rows.append(_np(r))
    return np.min(rows, axis=0)


@pytest.mark.parametrize("N", [1, 4])
def test_agent_with_the_real_world_as_its_only_member_is_the_safe_agent(N, tmp_path):
    from test_safe_ars_agent_cpu import DB
    H, iters = 100, 3
    w0 = str(tmp_path / "w0.npy")
    np.save(w0, np.random.RandomState(7).uniform(-1, 1, (2, 8)))
    ep, ap = _real(3, H), _agent_param(N, H, w0, iters)
    margin = Threshold(1, 0.3, 0.001)
    plain = sw.ARSAgent(copy.copy(ep), ap, data_path=DB, seed=4, sim_thresh=margin)
    ens = sw.ARSAgent(copy.copy(ep), ap, data_path=DB, seed=4, sim_thresh=margin, sim_ensemble=[copy.copy(ep)])
    assert ens.sim_threshold == plain.sim_threshold == ap.threshold + margin.compute_alpha(H) * ep.epsilon
    assert ens.estimated_param == ep and ens.estimated_param is not ep
    # a threshold that bites: in the middle of the first iteration's simulator returns (N = 4: a partial admission)
    w = _first_worst(plain, ap, [ep], 4)
    plain.sim_threshold = ens.sim_threshold = float(np.median(np.minimum(w[0::2], w[1::2])) + (1e-9 if N > 1 else -1e-9))
    runs = []
    for agent in (plain, ens):
        np.random.seed(4)
        admitted, inner = [], agent.runOneIteration

        def recorded(agent=agent, inner=inner, admitted=admitted):
            r = inner()
            admitted.append(agent.last_admitted.copy())
            return r
        agent.runOneIteration = recorded
        runs.append((agent.runTraining(), agent.policy, agent.mean, admitted, agent.violations))
    (c0, p0, m0, a0, v0), (c1, p1, m1, a1, v1) = runs
    assert np.array_equal(c0, c1, equal_nan=True) and np.array_equal(p0, p1) and np.array_equal(m0, m1) and v0 == v1
    assert len(a0) == len(a1) == iters + 1 and all(np.array_equal(x, y) for x, y in zip(a0, a1))
    assert len(a0[0]) == (2 if N == 4 else 1)               # by construction: the first iteration
    assert ens.last_worst.shape == (2 * N,) and np.isfinite(ens.last_worst).all()


def test_agent_with_three_members_and_no_threshold_object(tmp_path):
    from test_safe_ars_agent_cpu import DB
    N, H = 4, 100
    w0 = str(tmp_path / "w0.npy")
    np.save(w0, np.random.RandomState(7).uniform(-1, 1, (2, 8)))
    ep = _real(3, H)
    members = _ensemble(ep, 0)
    probe = sw.ARSAgent(copy.copy(ep), _agent_param(N, H, w0), data_path=DB, seed=4, sim_ensemble=members)
    worst = _first_worst(probe, probe.agent_param, members, 4)
    l = float(np.median(np.minimum(worst[0::2], worst[1::2])) + 1e-9)
    ap = _agent_param(N, H, w0, iters=4, threshold=l)
    agent = sw.ARSAgent(copy.copy(ep), ap, data_path=DB, seed=4, sim_ensemble=members)      # sim_thresh=None
    assert agent.sim_threshold == l and agent.estimated_param == members[0]
    np.random.seed(4)
    r = agent.runOneIteration()
    assert np.array_equal(agent.last_worst, worst)                   # the minimum of three single gates, bit for bit
    expect = np.flatnonzero(~(worst[0::2] <= l) & ~(worst[1::2] <= l))
    assert np.array_equal(agent.last_admitted, expect) and 0 < len(expect) < N and len(r) == 2 * len(expect)
    # it trains; an iteration the gate refuses altogether repeats the last mean in the curve, as runTraining does
    before = agent.policy
    per_it, inner = [], agent.runOneIteration

    def recorded():
        agent.sim_threshold = 1e9 if len(per_it) % 2 == 1 else -1e9   # every second iteration: all refused
        out = inner()
        per_it.append(out)
        return out
    agent.runOneIteration = recorded
    curve = agent.runTraining()
    assert not np.array_equal(agent.policy, before)
    assert len(per_it) == 5 and [len(x) == 0 for x in per_it[1::2]] == [True, True] and len(per_it[0]) > 0
    for j, x in enumerate(per_it):
        assert curve[j] == (np.mean(x) if len(x) else curve[j - 1])
    assert np.isinf(agent.last_worst).sum() == 0 and agent.last_worst.shape == (2 * N,)


@pytest.mark.parametrize("N", [1, 4])
def test_batch_with_ensembles_equals_independent_agents(N, tmp_path):
    from test_safe_ars_agent_cpu import DB
    S, H, iters = 3, 60, 4
    w0 = str(tmp_path / "w0.npy")
    np.save(w0, np.random.RandomState(7).uniform(-1, 1, (2, 8)))
    ep = _real(3, H)
    ap = _agent_param(N, H, w0, iters - 1)
    ensembles = [_ensemble(ep, a) for a in range(S)]
    agents = [sw.ARSAgent(copy.copy(ep), ap, data_path=DB, seed=s, sim_ensemble=ensembles[s], full_covariance=False)
              for s in range(S)]
    # agent 0 always admitted, agent 1 always refused, agent 2 in the middle of its first iteration's worst returns
    w = _first_worst(agents[2], ap, ensembles[2], 2)
    sim_thr = [-1e9, 1e9, float(np.median(np.minimum(w[0::2], w[1::2])) + (1e-9 if N > 1 else -1e-9))]
    record = []
    for s, agent in enumerate(agents):
        agent.sim_threshold = sim_thr[s]
        np.random.seed(s)
        rows = []
        for _ in range(iters):
            r = agent.runOneIteration()
            rows.append((r, agent.last_admitted.copy(), agent.policy, agent.mean, agent.last_worst.copy()))
        record.append(rows)
    batch = sw.SafeARSAgentBatch(ep, ap, range(S), None, sim_thr, sim_ensembles=ensembles)
    ks = set()
    for it in range(iters):
        rets = batch.runOneIteration()
        pol, mean = batch.policy, batch.mean
        for s in range(S):
            r, admitted, p1, m1, w1 = record[s][it]
            assert np.array_equal(rets[s], r), (it, s, "returns")
            assert np.array_equal(batch.last_admitted[s], admitted), (it, s, "admitted")
            assert np.array_equal(pol[s], p1), (it, s, "policy")
            assert np.array_equal(mean[s], m1), (it, s, "mean")
            assert np.array_equal(batch.last_worst[s], w1), (it, s, "worst")
            ks.add(len(admitted))
    assert np.array_equal(batch.violations, [a.violations for a in agents])
    assert 0 in ks and N in ks
    if N >= 2:
        assert any(0 < k < N for k in ks) and 0 < len(record[2][0][1]) < N      # partial admissions are present
    assert batch.min_admitted_worst[1] == np.inf and batch.min_admitted_worst[2] > sim_thr[2]


def test_run_ensemble_at_a_tiny_size(tmp_path, monkeypatch):
    eps, n_seed, n_sim, H, n_iter = (0.001, 0.01), 2, 3, 50, 3
    seen = []

    class Recording(sw.SafeARSAgentBatch):
        def _read(self, rows):
            out = super()._read(rows)
            seen.extend(out)
            return out
    monkeypatch.setattr(safe_exploration, "SafeARSAgentBatch", Recording)
    out = safe_exploration.run_ensemble(epsilons=eps, n_seed=n_seed, n_sim=n_sim, n_iter=n_iter, hand_iter=3, H=H,
                                        results_path=str(tmp_path / "results"), data_path=str(tmp_path / "data"),
                                        rng=np.random.RandomState(5), ensemble_rng=np.random.RandomState(6))
    assert {"l", "epsilons", "r_graphs", "min_return", "max_mean_returns", "sim_thresh_range", "sim_params",
            "violations", "worst_margin"} <= set(out) and "A_values" not in out
    assert out["r_graphs"].shape == (2, n_seed, n_iter + 1) and out["violations"].shape == (2, n_seed)
    for name in ("min_return", "max_mean_returns", "sim_thresh_range", "worst_margin"):
        assert np.shape(out[name]) == (2,), name
    l = out["l"]
    assert float(np.loadtxt(os.path.join(str(tmp_path / "data"), "threshold.txt"))) == pytest.approx(l, rel=1e-15)
    assert np.array_equal(out["sim_thresh_range"], [l, l])
    # the centres are run()'s simulators, the ensembles sphere_ensemble around them, drawn in agent order
    rng, ens_rng = np.random.RandomState(5), np.random.RandomState(6)
    k = 0
    for e in eps:
        for c in ars_agent.approximate_env_params(safe_exploration.real_world(H, e), e, n_seed, rng):
            assert out["sim_params"][k] == c
            assert out["sim_ensembles"][k] == sphere_ensemble(c, e, n_sim, ens_rng)
            k += 1
    # worst_margin > 0 wherever something was admitted, and every real return of an admitted direction is finite
    assert len(seen) == n_iter + 1
    admitted = np.array([[len(r) for r in per_agent] for per_agent in seen]).reshape(n_iter + 1, 2, n_seed)
    for i in range(2):
        if admitted[:, i].any():
            assert 0 < out["worst_margin"][i] < np.inf
        else:
            assert out["worst_margin"][i] == np.inf
    assert admitted.any()
    assert all(np.isfinite(r).all() for per_agent in seen for r in per_agent)


if __name__ == "__main__" and sys.argv[1:] == ["quad-child"]:
    # the child of test_the_quad_form_in_a_child_process
    _check_form(3, "auto")
    print("quad-child ok")
