"""CACLA behind the simulator gate without a GPU: the entry point's declaration, binding and argument checks, the
wrapper's parameter names, the classes' constructor errors, the reference's list rule, and the NumPy restatement
(tests/cacla_safe_oracle.py) against tests/cacla_oracle.py where the gate admits everything."""
import ctypes
import os

import numpy as np
import pytest
import torch

import swimmer_amd as sw
from conftest import ROOT
from swimmer_amd import cacla
from swimmer_amd.cacla import safe_kernels
from swimmer_amd.safe_ars import AbsObs, MaxAbsThetaDot

import cacla_oracle
import cacla_safe_oracle as oracle_se

HEADER = os.path.join(ROOT, "include", "swimmer_hip.h")


def test_entry_point_is_declared_exported_and_bound():
    src = open(HEADER).read()
    assert ("int sw_cacla_safe_run_f64(const sw_params *real, int64_t n_agent, int32_t n_iter, int64_t t_begin,"
            in src)
    assert "#define SW_ABI_VERSION 3\n" in src and sw._lib.ABI_VERSION == 3
    assert "sw_cacla_safe_run_f64" in sw._lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(sw._lib.library_path()), "sw_cacla_safe_run_f64")
    lib = sw._lib.load()
    assert lib.sw_abi_version() == 3
    assert len(lib.sw_cacla_safe_run_f64.argtypes) == 22
    assert "swimmer_cacla_safe.hip" in sw._build.SOURCES
    assert not hasattr(sw.kernels, "cacla_safe_run") and callable(safe_kernels.cacla_safe_run)
    assert cacla.CACLA_SE_agent and cacla.CACLA_SE_Batch and cacla.swimmer_experiment.safe_compare


REQUIRED = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13)   # of the 15 pointers from gamma on; 11 admitted_rec, 14 status


def test_entry_point_validates_without_gpu():
    fn = sw._lib.load().sw_cacla_safe_run_f64
    ok = sw.SwParams.make(3)
    dev = ctypes.c_void_p(8)          # never dereferenced: validation comes first

    def call(p, n_agent=5, n_iter=16, t_begin=0, kind=sw._lib.COST_MAX_ABS_THETADOT, index=0, missing=None):
        ptrs = [None if i == missing else dev for i in range(15)]
        return fn(ctypes.byref(p) if p is not None else None, n_agent, n_iter, t_begin, *ptrs[:7], kind, index,
                  *ptrs[7:], None)
    assert call(None) == 1
    for missing in REQUIRED:
        assert call(ok, missing=missing) == 1, missing
    assert call(ok, n_agent=0) == 3
    assert call(ok, n_agent=-4) == 3
    assert call(ok, n_agent=2 ** 31) == 3
    assert call(ok, n_iter=-1) == 3
    assert call(ok, t_begin=-1) == 3
    assert call(ok, t_begin=2 ** 31 - 16) == 3                          # t_begin + n_iter > 2^31 - 1: first_refused is int32
    assert call(ok, t_begin=2 ** 31 - 1, n_iter=1) == 3
    assert call(ok, t_begin=2 ** 40) == 3
    assert call(ok, t_begin=2 ** 31 - 1, n_iter=0) == 0                 # the last step count that fits, nothing to do
    assert call(ok, kind=2) == 3
    assert call(ok, kind=-1) == 3
    assert call(ok, kind=sw._lib.COST_ABS_OBS, index=8) == 3            # d = 8: 0..7
    assert call(ok, kind=sw._lib.COST_ABS_OBS, index=-1) == 3
    assert call(ok, kind=sw._lib.COST_MAX_ABS_THETADOT, index=99, n_iter=0) == 0   # the index is not read
    assert call(sw.SwParams.make(3, flags=4)) == 4                      # twin model
    assert call(sw.SwParams.make(9)) == 2
    assert call(sw.SwParams.make(1)) == 2
    assert call(ok, n_iter=0) == 0                                      # nothing to do, nothing written
    assert call(ok, n_iter=0, kind=sw._lib.COST_ABS_OBS, index=7) == 0
    assert call(ok, n_iter=0, missing=11) == 0 and call(ok, n_iter=0, missing=14) == 0   # the optional two


def _arguments(A=2, n_iter=5, n=3):
    p = sw.SwParams.make(n)
    f = lambda *shape: torch.zeros(shape, dtype=torch.float64)       # noqa: E731
    i = lambda *shape: torch.zeros(shape, dtype=torch.int32)         # noqa: E731
    return p, dict(gamma=f(A), alpha=f(A), noise=f(A, n_iter, p.m), gated=i(A), sim=f(A, 3), sim_thresh=f(A),
                   real_thresh=f(A), weights=f(A, n, cacla.net_doubles(n)), state=f(A, p.d), last_reward=f(A),
                   counters=i(A, 3), first_refused=i(A), rewards=f(A, n_iter), admitted_rec=i(A, n_iter), status=i(A))


BAD = {"alpha": torch.zeros(3, dtype=torch.float64), "noise": torch.zeros((2, 5, 3), dtype=torch.float64),
       "gated": torch.zeros(2, dtype=torch.float64), "sim": torch.zeros((2, 2), dtype=torch.float64),
       "sim_thresh": torch.zeros(2, dtype=torch.float32), "real_thresh": None,
       "weights": torch.zeros((2, 3, 10), dtype=torch.float64), "state": torch.zeros((8, 2), dtype=torch.float64).t(),
       "last_reward": torch.zeros((2, 1), dtype=torch.float64), "counters": torch.zeros((2, 3), dtype=torch.int64),
       "first_refused": torch.zeros(2, dtype=torch.float64), "rewards": torch.zeros((2, 6), dtype=torch.float64),
       "admitted_rec": torch.zeros((2, 5), dtype=torch.float64), "status": torch.zeros(3, dtype=torch.int32)}


@pytest.mark.parametrize("name", sorted(BAD))
def test_the_wrapper_names_the_bad_parameter(monkeypatch, name):
    """The checks run on CPU tensors here: the GPU requirement is taken out, and the foreign call is never reached."""
    monkeypatch.setattr(safe_kernels, "require_gpu", lambda: None)
    monkeypatch.setattr(safe_kernels, "_gpu", lambda t, name, ndim: (torch.device("cpu"), name))
    p, kw = _arguments()
    kw[name] = BAD[name]
    with pytest.raises(sw.SwimmerHipError, match=rf"^{name}: expected a contiguous .* as gamma, got "):
        safe_kernels.cacla_safe_run(p, 5, 0, cost_kind=1, cost_index=0, **kw)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal is what a machine without a GPU sees")
def test_without_a_gpu_the_wrapper_says_that_there_is_no_cpu_fallback():
    p, kw = _arguments()
    with pytest.raises(sw.SwimmerHipError, match="no CPU fallback"):
        safe_kernels.cacla_safe_run(p, 5, 0, cost_kind=1, cost_index=0, **kw)


def test_constructor_errors():
    sim = sw.SwimmerEnv(n=3)
    with pytest.raises(TypeError, match="NativeCost"):
        cacla.CACLA_SE_agent(0.9, 0.01, 1.0, sim, lambda obs: abs(obs[3]), 0.3, 0.2)
    with pytest.raises(TypeError, match="NativeCost"):
        cacla.CACLA_SE_Batch(sim, [0.9], [0.01], [1.0], [0], [(1, 1, 10)], [0.2], [0.3], abs)
    with pytest.raises(ValueError, match="same length"):
        cacla.CACLA_SE_Batch(sim, [0.9, 0.9], [0.01], [1.0], [0], [(1, 1, 10)], [0.2], [0.3], AbsObs(3))
    with pytest.raises(ValueError, match="same length"):
        cacla.CACLA_SE_Batch(sim, [0.9], [0.01], [1.0], [0], [(1, 1, 10)], [0.2], [0.3], AbsObs(3), gated=[1, 0])
    agent = cacla.CACLA_SE_agent(0.9, 0.01, 1.0, sim, MaxAbsThetaDot(), 0.3, 0.2)
    for other in (sw.SwimmerEnv(n=4), sw.SwimmerEnv(n=3, h=2e-3), sw.SwimmerEnv(n=3, direction=[0.0, 1.0])):
        with pytest.raises(ValueError, match="n, h and direction"):
            agent.run(other, 10)                            # refused before anything is drawn or launched
        with pytest.raises(ValueError, match="n, h and direction"):
            cacla.swimmer_experiment.safe_compare(other, sim, 0.9, 0.01, 1.0, [0], AbsObs(3), 0.3, 0.2, 10)


def test_the_reward_list_follows_the_references_append_rule():
    """cacla_safe_agent.py:177-188: nothing before the first admitted step, then one entry per step, a refused step
    repeating the last reward."""
    admitted = np.array([0, 0, 1, 0, 1, 1, 0], dtype=bool)
    rewards = np.array([np.nan, np.nan, 1.0, 1.0, 2.0, 3.0, 3.0])
    want = []
    for t in range(7):                                      # the reference's list, step by step
        if admitted[t]:
            want.append(rewards[t])
        elif want:
            want.append(want[-1])
    assert cacla.trim_rewards(rewards, admitted) == want == [1.0, 1.0, 2.0, 3.0, 3.0]
    assert oracle_se.trim(rewards, admitted) == want
    assert cacla.trim_rewards(np.full(4, np.nan), np.zeros(4, dtype=bool)) == []
    assert cacla.trim_rewards(np.arange(3.0), np.ones(3, dtype=bool)) == [0.0, 1.0, 2.0]
    assert cacla.trim_rewards(np.empty(0), np.empty(0, dtype=bool)) == []


@pytest.mark.parametrize("n", (2, 3, 6))
@pytest.mark.parametrize("how", ("gate wide open", "ungated"))
def test_the_oracle_with_nothing_refused_is_the_plain_oracle_exactly(n, how):
    rs = np.random.RandomState(n)
    w = rs.uniform(-0.3, 0.3, (n, cacla_oracle.net_doubles(n)))
    noise = rs.normal(0.0, 1.0, (40, n - 1))
    plain = cacla_oracle.run(n, 0.9, 0.05, w, noise)
    safe = oracle_se.run(n, 0.9, 0.05, w, noise, oracle_se.max_abs_thetadot, (1.02, 0.97, 10.3),
                         np.inf, 0.01, gated=(how == "gate wide open"))
    assert np.array_equal(safe["rewards"], plain["rewards"]) and np.array_equal(safe["weights"], plain["weights"])
    assert np.array_equal(safe["state"], plain["state"])
    assert safe["admitted"].all() and safe["first_refused"] is None
    assert safe["counters"][0] == 40 and safe["counters"][2] == plain["actor_updates"]
    assert safe["min_td"] == plain["min_td"]
    assert safe["counters"][1] > 0                          # a real threshold of 0.01 is crossed with this noise


def test_the_oracle_refuses_on_nan_and_keeps_everything():
    n = 3
    rs = np.random.RandomState(3)
    w = rs.uniform(-0.3, 0.3, (n, cacla_oracle.net_doubles(n)))
    got = oracle_se.run(n, 0.9, 0.05, w, rs.normal(0.0, 1.0, (10, n - 1)), oracle_se.abs_obs(3), (1.0, 1.0, 10.0),
                        np.nan, 0.1)
    assert np.isnan(got["rewards"]).all() and not got["admitted"].any() and got["first_refused"] == 0
    assert got["counters"] == (0, 0, 0) and np.array_equal(got["weights"], w)
    assert oracle_se.trim(got["rewards"], got["admitted"]) == []
