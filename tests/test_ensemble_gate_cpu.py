"""The ensemble gate's host side without a GPU: the entry point exists and checks its arguments before any HIP call,
sphere_ensemble / ensemble_from_estimates build what they say, fold_reference is the rule of ars/ensemble.py on
hand-made arrays, the wrapper names the parameter it refuses, and the agents refuse bad ensembles before touching the
device."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import swimmer_amd as sw
from swimmer_amd.ars import ensemble, ensemble_kernels
from swimmer_amd.ars.parameters import Threshold
from conftest import GOLDEN

NAME = "sw_ars_gate_ensemble_f64"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swimmer_hip.h")
DB = os.path.join(GOLDEN, "safe_agent_db.npz")
NAN, INF = float("nan"), float("inf")


def test_entry_point_is_declared_exported_and_the_abi_version_stays():
    with open(HEADER) as f:
        text = f.read()
    lib = sw._lib.load()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", text)
    assert NAME in sw._lib.EXPORTED_SYMBOLS
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 19
    assert fn.argtypes[1:5] == [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]
    assert fn.argtypes[7] is ctypes.c_double
    assert sw._lib.ABI_VERSION == 3 and lib.sw_abi_version() == 3 and "#define SW_ABI_VERSION 3" in text


def test_entry_point_validates_before_any_device_work():
    lib = sw._lib.load()
    ok, P = ctypes.byref(sw.SwParams.make(3)), ctypes.c_void_p(8)      # P: non-NULL, never dereferenced
    bad_n, bad_l = ctypes.byref(sw.SwParams.make(9)), ctypes.byref(sw.SwParams.make(3, l_i=-1.0))
    gate = getattr(lib, NAME)

    # (every call below fails a check: none reaches a launch)
    def g(p=ok, S=2, E=3, N=1, H=5, policy=P, deltas=P, mean=None, inv_std=None, sim=P, thr=P, admit=P, worst=P,
          status=None, m_ret=P, m_st=P, m_adm=P):
        return gate(p, S, E, N, H, policy, deltas, 0.01, mean, inv_std, sim, thr, admit, worst, status, m_ret, m_st,
                    m_adm, None)
    assert g(p=None) == 1
    assert g(S=0) == 3 and g(E=0) == 3 and g(N=0) == 3 and g(H=-1) == 3 and g(S=-1) == 3 and g(E=-1) == 3
    assert g(S=65536, E=1) == 3 and g(S=1, E=65536) == 3 and g(S=256, E=256) == 3      # the product: 65536
    assert g(S=2 ** 40, E=2 ** 40) == 3                                                 # no overflow into range
    assert g(N=2 ** 23 + 1) == 3
    assert g(S=255, E=257, N=2 ** 23) == 3                                              # 2^32 threads and more
    for name in ("policy", "deltas", "sim", "thr", "admit", "worst", "m_ret", "m_st", "m_adm"):
        assert g(**{name: None}) == 1, name
    assert g(S=255, E=257, policy=None) == 1                                            # 65535 members: in range
    assert g(mean=P) == 1 and g(inv_std=P) == 1                                         # one without the other
    assert g(p=bad_n) == 2 and g(p=bad_l) == 4


# ---- the ensembles ----------------------------------------------------------------------------------------------
def _real(H=200):
    return sw.EnvParam("LeonSwimmer-RealWorld", n=3, H=H, l_i=.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0.001)


def _unknowns(p):
    return np.array([p.m_i, p.l_i, p.k])


def test_sphere_ensemble_puts_its_members_on_the_sphere_in_member_order():
    """The distance bound.  A member is stored as centre + step, coordinate by coordinate, so what can be read back
    is the step rounded to the coordinate's grid: at most half an ulp of the coordinate off per coordinate, at most
    half an ulp of the LARGEST coordinate (k) off in the norm, plus a few ulp of epsilon from the normalisation,
    which is smaller still.  The test allows 4 ulp of that coordinate."""
    centre, eps, E = _real(), 0.005, 6
    before = copy.copy(centre)
    members = ensemble.sphere_ensemble(centre, eps, E, np.random.RandomState(3))
    assert centre == before and len(members) == E
    assert members[0] == centre and members[0] is not centre
    ulp = np.spacing(np.abs(_unknowns(centre)).max())
    rng = np.random.RandomState(3)
    for i in range(1, E):
        m = members[i]
        assert (m.n, m.H, m.h, m.epsilon, m.name) == (centre.n, centre.H, centre.h, centre.epsilon, centre.name)
        d = _unknowns(m) - _unknowns(centre)
        off = abs(np.linalg.norm(d) - eps)
        print(f"member {i}: | ||d|| - eps | = {off / ulp:.3f} ulp of k")
        assert off <= 4 * ulp
        g = rng.standard_normal(3)                                   # the draws, in member order
        assert np.array_equal(_unknowns(m), _unknowns(centre) + eps * (g / np.linalg.norm(g)))
    assert len({tuple(_unknowns(m)) for m in members}) == E
    again = ensemble.sphere_ensemble(centre, eps, E, np.random.RandomState(3))
    assert again == members
    np.random.seed(3)                                                # the default generator is NumPy's global one
    assert ensemble.sphere_ensemble(centre, eps, E) == members
    assert ensemble.sphere_ensemble(centre, eps, 1) == [centre]
    with pytest.raises(ValueError):
        ensemble.sphere_ensemble(centre, eps, 0)


def test_ensemble_from_estimates_drops_the_rows_that_break_the_parameter_rule():
    like = _real()
    good = copy.copy(like)
    good.l_i = 0.79
    bad = [copy.copy(like) for _ in range(4)]
    bad[0].m_i, bad[1].l_i, bad[2].k, bad[3].l_i = -1.0, 0.0, NAN, INF
    got = ensemble.ensemble_from_estimates([bad[0], like, bad[1], good, bad[2], bad[3]])
    assert got == [like, good] and got[0] is not like
    rows = [[1.2, 0.8, 10.2], [-1.0, 0.8, 10.2], [1.19, 0.81, 10.1], [1.2, 0.8, INF]]      # [m_i, l_i, k]
    got = ensemble.ensemble_from_estimates(rows, like=like)
    assert [(e.m_i, e.l_i, e.k) for e in got] == [(1.2, 0.8, 10.2), (1.19, 0.81, 10.1)]
    assert all((e.n, e.H, e.h) == (like.n, like.H, like.h) for e in got)
    with pytest.raises(ValueError, match="like"):
        ensemble.ensemble_from_estimates(rows)
    with pytest.raises(ValueError, match="parameter rule"):
        ensemble.ensemble_from_estimates(bad)
    with pytest.raises(ValueError, match="parameter rule"):
        ensemble.ensemble_from_estimates([])


# ---- the fold ---------------------------------------------------------------------------------------------------
def _invariant(admit, worst, status, thr):
    clean = (status[..., 0::2] | status[..., 1::2]) == 0
    with np.errstate(invalid="ignore"):
        by_worst = ~(worst[..., 0::2] <= thr) & ~(worst[..., 1::2] <= thr)
    return np.array_equal(admit.astype(bool)[clean], by_worst[clean])


def test_fold_reference_on_hand_made_members():
    thr = 3.0
    # E = 3 members, N = 6 directions; columns (r+, r-) per direction
    r = np.array([
        #  d0: all above   d1: one equal   d2: NaN among    d3: all NaN   d4: one below    d5: NaN and below
        [5.0, 6.0,         4.0, 3.0,       NAN, 7.0,        NAN, NAN,     4.0, 4.0,        NAN, 9.0],
        [4.0, 9.0,         4.0, 5.0,       4.5, NAN,        NAN, NAN,     2.0, 4.0,        8.0, NAN],
        [7.0, 3.5,         8.0, 5.0,       6.0, 3.5,        NAN, NAN,     4.0, 4.0,        2.5, 9.5],
    ])
    st = np.zeros(r.shape, dtype=np.int32)
    st[0, 4], st[2, 4], st[1, 5] = 2, 4, 1                            # direction 2: +, OR of two codes; - one code
    m_adm, admit, worst, status = ensemble.fold_reference(r, st, thr)
    assert m_adm.dtype == admit.dtype == status.dtype == np.int32 and m_adm.shape == (3, 6)
    assert m_adm.tolist() == [[1, 0, 1, 1, 1, 1], [1, 1, 1, 1, 0, 1], [1, 1, 1, 1, 1, 0]]
    assert admit.tolist() == [1, 0, 1, 1, 0, 0]                       # equality refuses; all-NaN admits
    assert worst.tolist() == [4.0, 3.5, 4.0, 3.0, 4.5, 3.5, INF, INF, 2.0, 4.0, 2.5, 9.0]
    assert status.tolist() == [0, 0, 0, 0, 6, 1, 0, 0, 0, 0, 0, 0]
    assert _invariant(admit, worst, status, thr)
    # a NaN threshold admits everything, -inf too, and the invariant holds for both
    for t in (NAN, -INF):
        _, a, w, s = ensemble.fold_reference(r, st, t)
        assert a.all() and np.array_equal(w, worst) and _invariant(a, w, s, t)
    # the order of the members does not matter to the minimum, NaN first or last
    _, _, w2, _ = ensemble.fold_reference(r[::-1], st[::-1], thr)
    assert np.array_equal(w2, worst)


def test_fold_reference_a_member_with_the_parameter_status_refuses_everything():
    r = np.array([[5.0, 6.0, 7.0, 8.0], [NAN, NAN, NAN, NAN], [5.5, 6.5, 7.5, 8.5]])
    st = np.zeros(r.shape, dtype=np.int32)
    st[1] = sw._lib.STATUS_PARAM
    m_adm, admit, worst, status = ensemble.fold_reference(r, st, 1.0)
    assert m_adm.tolist() == [[1, 1], [0, 0], [1, 1]] and not admit.any()
    assert worst.tolist() == [5.0, 6.0, 7.0, 8.0] and (status == sw._lib.STATUS_PARAM).all()
    assert _invariant(admit, worst, status, 1.0)                      # vacuous there: no direction has a clean status


def test_fold_reference_with_agent_axes_and_per_agent_thresholds():
    rng = np.random.RandomState(0)
    r = rng.uniform(0, 10, (4, 5, 12))
    r[rng.rand(*r.shape) < 0.15] = NAN
    st = (rng.rand(*r.shape) < 0.1).astype(np.int32) * rng.choice([1, 2, 4], r.shape)
    thr = np.array([2.0, NAN, -INF, 5.0])
    m_adm, admit, worst, status = ensemble.fold_reference(r, st, thr)
    assert m_adm.shape == (4, 5, 6) and admit.shape == (4, 6) and worst.shape == status.shape == (4, 12)
    for a in range(4):
        one = ensemble.fold_reference(r[a], st[a], thr[a])
        for got, ref in zip((m_adm[a], admit[a], worst[a], status[a]), one):
            assert np.array_equal(got, ref)
        assert _invariant(admit[a], worst[a], status[a], thr[a])
        assert np.array_equal(worst[a], np.where(np.isnan(r[a]).all(axis=0), INF, np.nanmin(
            np.where(np.isnan(r[a]), INF, r[a]), axis=0)))
        assert np.array_equal(status[a], np.bitwise_or.reduce(st[a], axis=0))
    assert admit[1].all() and admit[2].all() and 0 < admit[0].sum() + admit[3].sum() < 12


# ---- the wrapper ------------------------------------------------------------------------------------------------
def test_the_wrapper_names_the_parameter_it_refuses(monkeypatch):
    """On CPU tensors, with the GPU requirement taken out: every miss is caught by the shared checks before the
    library is reached (a call that passed them all would hand the library host pointers: none is made)."""
    cpu = torch.device("cpu")
    monkeypatch.setattr(ensemble_kernels, "require_gpu", lambda: None)
    monkeypatch.setattr(ensemble_kernels, "_gpu", lambda t, name, ndim: (cpu, name))
    monkeypatch.setattr(ensemble_kernels, "load", lambda: pytest.fail("the library must not be reached"))
    p = sw.SwParams.make(3)
    S, E, N, m, d = 2, 3, 4, 2, 8
    f64, i32 = torch.float64, torch.int32

    def call(**over):
        kw = dict(policy=torch.zeros((S, m, d), dtype=f64), deltas=torch.zeros((S, N, m, d), dtype=f64),
                  sim=torch.ones((S, E, 3), dtype=f64), sim_thresh=torch.zeros(S, dtype=f64))
        kw.update(over)
        return ensemble_kernels.ars_gate_ensemble(p, 5, kw.pop("policy"), kw.pop("deltas"), 0.01, kw.pop("sim"),
                                                  kw.pop("sim_thresh"), **kw)
    bad = {
        "policy": torch.zeros((S, m, d + 1), dtype=f64),
        "deltas": torch.zeros((S + 1, N, m, d), dtype=f64),
        "sim": torch.ones((S, 3), dtype=f64),                                   # the ensemble axis is missing
        "sim_thresh": torch.zeros((S, E), dtype=f64),                           # per agent, not per member
        "admit": torch.zeros((S, N), dtype=f64),                                # wrong dtype
        "worst": torch.zeros((S, N), dtype=f64),                                # [S, 2N]
        "status": torch.zeros((S, 2 * N), dtype=torch.int64),
        "member_returns": torch.zeros((S, 2 * N, E), dtype=f64).transpose(1, 2),    # right shape, not contiguous
        "member_status": torch.zeros((S, E, N), dtype=i32),
        "member_admit": torch.zeros((S * E, N), dtype=i32),                     # flat
    }
    for name, t in bad.items():
        with pytest.raises(sw.SwimmerHipError, match=rf"^{name}: expected a contiguous "):
            call(**{name: t})
    for name, t in (("sim", torch.ones((S + 1, E, 3), dtype=f64)), ("sim", torch.ones((S, E, 3), dtype=torch.float32)),
                    ("sim_thresh", torch.zeros(S, dtype=f64, device="meta")),
                    ("worst", torch.zeros((S, 2 * N + 1), dtype=f64)),
                    ("member_admit", torch.zeros((S, E, N), dtype=torch.int64)),
                    ("member_admit", torch.zeros((S, E + 1, N), dtype=i32))):
        with pytest.raises(sw.SwimmerHipError, match=rf"^{name}: "):
            call(**{name: t})
    with pytest.raises(sw.SwimmerHipError, match=r"^inv_std: "):
        call(mean=torch.zeros((S, d), dtype=f64))
    with pytest.raises(sw.SwimmerHipError, match=r"^mean: "):
        call(mean=torch.zeros((S, d + 1), dtype=f64), inv_std=torch.ones((S, d), dtype=f64))


def test_without_a_gpu_the_wrapper_says_that_there_is_no_cpu_fallback():
    if torch.cuda.is_available():
        return
    with pytest.raises(sw.SwimmerHipError, match="no CPU fallback"):
        ensemble_kernels.ars_gate_ensemble(sw.SwParams.make(3), 5, None, None, 0.01, None, None)


def test_the_wrapper_is_not_a_new_public_name_of_the_kernels_module():
    assert not hasattr(sw.kernels, "ars_gate_ensemble")


# ---- the agents' constructors -----------------------------------------------------------------------------------
def _agent_params(safe=True, N=2):
    return sw.ARSParam("S" if safe else "U", V1=True, n_iter=1, H=200, N=N, b=N, alpha=0.01, nu=0.01, safe=safe,
                       threshold=0.0, initial_w="Zero")


def _forbid_gpu(monkeypatch):
    from swimmer_amd.ars import ars_agent, safe_agent_batch

    def reached():
        raise AssertionError("the GPU was asked for before the arguments were refused")
    monkeypatch.setattr(ars_agent, "require_gpu", reached)
    monkeypatch.setattr(safe_agent_batch, "require_gpu", reached)


def test_agent_refuses_a_bad_ensemble_before_touching_the_gpu(monkeypatch):
    _forbid_gpu(monkeypatch)
    ep, ap = _real(), _agent_params()
    ens = [copy.copy(ep), copy.copy(ep)]
    other = dict(n=sw.EnvParam("Sim", n=4, H=200, l_i=.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0.001),
                 h=sw.EnvParam("Sim", n=3, H=200, l_i=.8, m_i=1.2, h=2e-3, k=10.2, epsilon=0.001),
                 H=sw.EnvParam("Sim", n=3, H=100, l_i=.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0.001))
    for what, member in other.items():
        with pytest.raises(ValueError, match=r"sim_ensemble\[1\]"):
            sw.ARSAgent(ep, ap, data_path=DB, seed=0, sim_ensemble=[ens[0], member])
    with pytest.raises(ValueError, match="at least one"):
        sw.ARSAgent(ep, ap, data_path=DB, seed=0, sim_ensemble=[])
    with pytest.raises(ValueError, match="safe"):
        sw.ARSAgent(ep, _agent_params(safe=False), seed=0, sim_ensemble=ens)
    with pytest.raises(ValueError, match="guess_param"):
        sw.ARSAgent(ep, ap, data_path=DB, seed=0, sim_ensemble=ens, guess_param=copy.copy(ep))
    with pytest.raises(ValueError, match="approx_error"):
        sw.ARSAgent(ep, ap, data_path=DB, seed=0, sim_ensemble=ens, approx_error=1e-3)
    with pytest.raises(ValueError, match="data_path"):
        sw.ARSAgent(ep, ap, seed=0, sim_ensemble=ens)
    with pytest.raises(ValueError, match="data_path"):
        sw.ARSAgent(ep, ap, seed=0, sim_ensemble=ens, sim_thresh=Threshold(1, 0.3, 0.001))


def test_sim_thresh_none_without_an_ensemble_still_raises(monkeypatch):
    _forbid_gpu(monkeypatch)
    with pytest.raises(ValueError, match="sim_thresh"):
        sw.ARSAgent(_real(), _agent_params(), data_path=DB, seed=0)
    with pytest.raises(ValueError, match="data_path"):
        sw.ARSAgent(_real(), _agent_params(), seed=0, sim_thresh=Threshold(1, 0.3, 0.001))


def test_batch_refuses_bad_ensembles_before_touching_the_gpu(monkeypatch):
    _forbid_gpu(monkeypatch)
    ep, ap = _real(), _agent_params()
    two = [copy.copy(ep), copy.copy(ep)]
    with pytest.raises(ValueError, match="not both"):
        sw.SafeARSAgentBatch(ep, ap, [0, 1], two, [0.0, 0.0], sim_ensembles=[two, two])
    with pytest.raises(ValueError, match="sim_params or sim_ensembles"):
        sw.SafeARSAgentBatch(ep, ap, [0, 1], None, [0.0, 0.0])
    with pytest.raises(ValueError, match="2 sim_ensembles"):
        sw.SafeARSAgentBatch(ep, ap, [0, 1], None, [0.0, 0.0], sim_ensembles=[two])
    with pytest.raises(ValueError, match="share the ensemble size"):
        sw.SafeARSAgentBatch(ep, ap, [0, 1], None, [0.0, 0.0], sim_ensembles=[two, two[:1]])
    with pytest.raises(ValueError, match="at least one"):
        sw.SafeARSAgentBatch(ep, ap, [0, 1], None, [0.0, 0.0], sim_ensembles=[[], []])
    other_H = sw.EnvParam("Sim", n=3, H=100, l_i=.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0.001)
    with pytest.raises(ValueError, match=r"sim_ensembles\[1\]\[0\]"):
        sw.SafeARSAgentBatch(ep, ap, [0, 1], None, [0.0, 0.0], sim_ensembles=[two, [other_H, two[0]]])
    with pytest.raises(ValueError, match="sim_thresholds"):
        sw.SafeARSAgentBatch(ep, ap, [0, 1], None, [0.0], sim_ensembles=[two, two])
    with pytest.raises(ValueError, match="safe"):
        sw.SafeARSAgentBatch(ep, _agent_params(safe=False), [0, 1], None, [0.0, 0.0], sim_ensembles=[two, two])
