"""The safe batch's host side without a GPU: the four entry points exist and check their arguments before any HIP
call, approximate_env_params draws what each agent's approximation branch draws, and SafeARSAgentBatch refuses what
it does not support before touching the device."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import swimmer_amd as sw
from swimmer_amd.ars import ars_agent
from conftest import GOLDEN

NEW = ("sw_ars_gate_multi_f64", "sw_ars_pack_admitted_f64", "sw_ars_rollouts_multi_counted_f64",
       "sw_ars_update_multi_counted_f64")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swimmer_hip.h")


def test_entry_points_are_declared_exported_and_the_abi_version_stays():
    with open(HEADER) as f:
        text = f.read()
    lib = sw._lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in sw._lib.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert sw._lib.ABI_VERSION == 3
    assert lib.sw_abi_version() == 3
    assert "#define SW_ABI_VERSION 3" in text


def test_entry_points_validate_before_any_device_work():
    lib = sw._lib.load()
    ok, P = ctypes.byref(sw.SwParams.make(3)), ctypes.c_void_p(8)      # P: non-NULL, never dereferenced
    bad_n, bad_l = ctypes.byref(sw.SwParams.make(9)), ctypes.byref(sw.SwParams.make(3, l_i=-1.0))
    # (every call below fails a check: none reaches a launch)
    gate = lib.sw_ars_gate_multi_f64

    def g(p=ok, S=2, N=1, H=5, policy=P, deltas=P, mean=None, inv_std=None, sim=P, thr=P, admit=P, returns=P):
        #           base S  N  H  policy  deltas  nu    mean  inv_std  sim  thresh admit  returns status stream
        return gate(p, S, N, H, policy, deltas, 0.01, mean, inv_std, sim, thr, admit, returns, None, None)
    assert g(p=None) == 1
    assert g(S=0) == 3 and g(S=65536) == 3 and g(N=0) == 3 and g(H=-1) == 3
    for name in ("policy", "deltas", "sim", "thr", "admit", "returns"):
        assert g(**{name: None}) == 1, name
    assert g(mean=P) == 1 and g(inv_std=P) == 1                        # one without the other
    assert g(p=bad_n) == 2 and g(p=bad_l) == 4

    pack = lib.sw_ars_pack_admitted_f64

    def k(p=ok, S=2, N=1, admit=P, deltas=P, count=P, order=P, packed=P):
        #           p  S  N  admit  status deltas  count  order  packed  stream
        return pack(p, S, N, admit, None, deltas, count, order, packed, None)
    assert k(p=None) == 1
    assert k(S=0) == 3 and k(S=65536) == 3 and k(N=0) == 3
    for name in ("admit", "deltas", "count", "order", "packed"):
        assert k(**{name: None}) == 1, name
    assert k(p=bad_n) == 2 and k(p=bad_l) == 4

    roll = lib.sw_ars_rollouts_multi_counted_f64

    def r(p=ok, S=2, N=1, count=P, H=5, policy=P, deltas=P, mean=None, inv_std=None, returns=P):
        #           p  S  N  count  H  policy  deltas  nu    mean  inv_std  returns moments status stream
        return roll(p, S, N, count, H, policy, deltas, 0.01, mean, inv_std, returns, None, None, None)
    assert r(p=None) == 1
    assert r(S=0) == 3 and r(S=65536) == 3 and r(N=0) == 3 and r(H=-1) == 3
    for name in ("count", "policy", "deltas", "returns"):
        assert r(**{name: None}) == 1, name
    assert r(mean=P) == 1 and r(inv_std=P) == 1
    assert r(p=bad_n) == 2 and r(p=bad_l) == 4

    upd = lib.sw_ars_update_multi_counted_f64

    def u(p=ok, S=2, N=1, count=P, H=5, returns=P, deltas=P, policy=P, top_b=0, moments=None, rows=0, running=None,
          mean=None, inv_std=None):
        #          p  S  N  count  H  returns  deltas  policy  alpha b    top_b  moments  rows  running  mean  inv_std
        return upd(p, S, N, count, H, returns, deltas, policy, 0.01, 1.0, top_b, moments, rows, running, mean, inv_std,
                   None, None)                                        # sigma_out, stream
    assert u(p=None) == 1
    assert u(S=0) == 3 and u(S=65536) == 3 and u(N=0) == 3 and u(H=-1) == 3 and u(top_b=-1) == 3
    for name in ("count", "returns", "deltas", "policy"):
        assert u(**{name: None}) == 1, name
    assert u(running=P, rows=1, mean=P, inv_std=P) == 1                # running without moments
    assert u(running=P, moments=P, rows=0, mean=P, inv_std=P) == 3     # fewer moment rows than 2N rollouts fill
    assert u(p=bad_n) == 2 and u(p=bad_l) == 4


def _env():
    return sw.EnvParam("LeonSwimmer-RealWorld", n=3, H=200, l_i=.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0.001)


def test_approximate_env_params_draws_agent_by_agent_and_leaves_its_argument_alone():
    g = np.load(os.path.join(GOLDEN, "safe_agent.npz"), allow_pickle=False)
    n, V1, N, b, H, seed, iters, gseed, exact = (int(x) for x in g["a_cfg"])
    l_i, m_i, k, h, eps = g["a_phys"][:5]
    assert gseed == 11 and not exact
    ep = sw.EnvParam("LeonSwimmer-RealWorld", n=n, H=H, l_i=l_i, m_i=m_i, h=h, k=k, epsilon=eps)
    before = copy.copy(ep)
    sims = ars_agent.approximate_env_params(ep, eps, 3, rng=np.random.RandomState(11))
    assert ep == before and len(sims) == 3 and all(s is not ep for s in sims)
    # agent 0: the reference's own numbers, and approximate_env_param on a copy under the same state
    assert np.array_equal([sims[0].l_i, sims[0].m_i, sims[0].k, sims[0].h], g["a_estimated"])
    np.random.seed(11)
    one = ars_agent.approximate_env_param(copy.copy(ep), eps)
    assert sims[0] == one and sims[0].name == "LeonSwimmer-Simulator"
    # the later agents consume the stream in order: agent s is the s-th consecutive call on a fresh copy
    for s in (1, 2):
        assert sims[s] == ars_agent.approximate_env_param(copy.copy(ep), eps)
    assert len({(s.l_i, s.m_i, s.k) for s in sims}) == 3
    # the default generator is NumPy's global one
    np.random.seed(11)
    assert ars_agent.approximate_env_params(ep, eps, 3) == sims
    for s in sims:
        d = np.array([s.m_i - ep.m_i, s.l_i - ep.l_i, s.k - ep.k])
        assert abs(np.linalg.norm(d) - eps) < 1e-12


def test_safe_batch_refuses_what_it_does_not_support_before_touching_the_gpu():
    ep = _env()
    kw = dict(V1=True, n_iter=1, H=10, N=2, b=2, alpha=0.01, nu=0.01, threshold=0.0, initial_w="Zero")
    safe, unsafe = sw.ARSParam("S", safe=True, **kw), sw.ARSParam("U", safe=False, **kw)
    sims = [copy.copy(ep), copy.copy(ep)]
    with pytest.raises(ValueError, match="safe"):
        sw.SafeARSAgentBatch(ep, unsafe, [0, 1], sims, [0.0, 0.0])
    with pytest.raises(ValueError, match="seed"):
        sw.SafeARSAgentBatch(ep, safe, [], [], [])
    with pytest.raises(ValueError, match="sim_params"):
        sw.SafeARSAgentBatch(ep, safe, [0, 1], sims[:1], [0.0, 0.0])
    with pytest.raises(ValueError, match="sim_thresholds"):
        sw.SafeARSAgentBatch(ep, safe, [0, 1], sims, [0.0])
    with pytest.raises(ValueError, match="thresholds"):
        sw.SafeARSAgentBatch(ep, safe, [0, 1], sims, [0.0, 0.0], thresholds=[1.0])
    other_n = sw.EnvParam("Sim", n=4, H=200, l_i=.8, m_i=1.2, h=1e-3, k=10.2, epsilon=0.001)
    with pytest.raises(ValueError, match=r"sim_params\[1\]"):
        sw.SafeARSAgentBatch(ep, safe, [0, 1], [sims[0], other_n], [0.0, 0.0])
    other_h = sw.EnvParam("Sim", n=3, H=200, l_i=.8, m_i=1.2, h=2e-3, k=10.2, epsilon=0.001)
    with pytest.raises(ValueError, match=r"sim_params\[0\]"):
        sw.SafeARSAgentBatch(ep, safe, [0, 1], [other_h, sims[1]], [0.0, 0.0])
    with pytest.raises(ValueError, match="top_b"):
        sw.SafeARSAgentBatch(ep, safe, [0, 1], sims, [0.0, 0.0], top_b=-1)
    # the unsafe batch and the experiment stay as they were
    with pytest.raises(NotImplementedError):
        sw.ARSAgentBatch(ep, safe, [0, 1])
    assert sw.Experiment(ep).batched(safe) is False
