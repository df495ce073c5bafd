"""safe_ars/experiment.py as one batch, without a GPU: the CPU restatement of the experiment reproduces the reference
fixture, `experiment.draw_setup` draws theta_sim and the chained seeds as the script does, the entry point exists and
checks its arguments before any HIP call, and ARSBatch refuses what it cannot run before touching the device."""
import ctypes
import os
import re

import numpy as np
import pytest

import swimmer_amd as sw
from swimmer_amd.safe_ars import experiment
from conftest import GOLDEN
import safe_experiment_oracle as seo

NAME = "sw_safe_ars_rollouts_multi_f64"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swimmer_hip.h")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "safe_experiment.npz"), allow_pickle=False)


def test_the_restated_experiment_reproduces_the_reference(g):
    n, n_iter, N, b, H = (int(x) for x in g["a_cfg"])
    alpha, nu, thresh, sim_thresh = g["a_hyper"]
    for k, seed in enumerate(g["a_seeds"]):
        unsafe, safe = seo.experience(g["a_theta_real"], g["a_theta_sim"], thresh, sim_thresh, n_iter, N, b, alpha, nu,
                                      H, int(seed), n=n)
        # discrete outcomes: equal
        assert np.array_equal(safe["first_refused"], g["a_safe_first_refused"][k])
        assert safe["violations"].sum() == g["a_safe_violations"][k] == 4
        assert np.all(unsafe["first_refused"] == H)
        refused = safe["first_refused"].reshape(n_iter, 2 * N) < H
        assert refused.any(axis=1).all() and (~refused).any(axis=1).all()
        # the bars of the oracle's own training test (tests/test_oracle_golden.py, safe_train)
        for kind, r in (("unsafe", unsafe), ("safe", safe)):
            assert np.abs(r["policy"] - g[f"a_{kind}_policy"][k]).max() <= 1e-9, kind
            assert np.abs(r["curve"] - g[f"a_{kind}_returns"][k]).max() <= 1e-12, kind
            assert np.abs(r["script_costs"] - g[f"a_{kind}_costs"][k]).max() <= 1e-9, kind
            assert np.abs(r["costs"].max(axis=1) - g[f"a_{kind}_cost_max"][k]).max() <= 1e-9, kind
    assert g["a_unsafe_cost_max"].max(axis=1).round(2).tolist() == [1.26, 1.69]


def test_draw_setup_chains_the_seeds_and_leaves_the_global_generator_as_the_script_does(g):
    n, n_iter, N, b, H, n_seeds, global_seed = (int(x) for x in g["c_cfg"])
    epsilon = g["c_hyper"][3]
    state = np.random.get_state()
    try:
        np.random.seed(global_seed)
        theta_sim, seeds = experiment.draw_setup(epsilon, n_iter, N, n_seeds)
        assert np.array_equal(theta_sim, g["c_theta_sim"])
        assert seeds == g["c_seeds"].tolist()
        assert np.random.randint(2**32 - 1) == int(g["c_next_draw"])
        # given values are used as they are and draw nothing
        np.random.seed(global_seed)
        before = np.random.get_state()[1].copy()
        t2, s2 = experiment.draw_setup(epsilon, n_iter, N, 2, seeds=[7, 8], theta_sim=[1.0, 1.1, 10.0])
        assert s2 == [7, 8] and t2.tolist() == [1.0, 1.1, 10.0]
        assert np.array_equal(np.random.get_state()[1], before)
        with pytest.raises(ValueError, match="seeds"):
            experiment.draw_setup(epsilon, n_iter, N, 3, seeds=[7, 8], theta_sim=t2)
    finally:
        np.random.set_state(state)


def test_entry_point_is_declared_exported_and_the_abi_version_stays():
    with open(HEADER) as f:
        text = f.read()
    lib = sw._lib.load()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", text)
    assert NAME in sw._lib.EXPORTED_SYMBOLS
    assert getattr(lib, NAME) is not None
    assert sw._lib.ABI_VERSION == 3 and lib.sw_abi_version() == 3
    assert "#define SW_ABI_VERSION 3" in text
    assert callable(sw.kernels.safe_ars_rollouts_multi) and sw.safe_ars.ARSBatch is not None


def test_entry_point_validates_before_any_device_work():
    fn = sw._lib.load().sw_safe_ars_rollouts_multi_f64
    ok, P = ctypes.byref(sw.SwParams.make(3)), ctypes.c_void_p(8)      # P: non-NULL, never dereferenced
    bad_n, bad_l = ctypes.byref(sw.SwParams.make(9)), ctypes.byref(sw.SwParams.make(3, l_i=-1.0))

    def f(p=ok, A=2, N=1, H=5, policy=P, deltas=P, gated=P, sim=P, sim_thr=P, real_thr=P, kind=1, index=0, returns=P):
        #         real A  N  H  policy  deltas  nu   gated  sim  sim_thresh real_thresh kind  index  returns
        return fn(p, A, N, H, policy, deltas, 0.5, gated, sim, sim_thr, real_thr, kind, index, returns,
                  None, None, None, None, None, None)          # cost_trace .. status, stream
    # (every call below fails a check: none reaches a launch)
    assert f(p=None) == 1
    assert f(A=0) == 3 and f(A=65536) == 3 and f(N=0) == 3 and f(N=(1 << 23) + 1) == 3 and f(H=-1) == 3
    assert f(kind=2) == 3 and f(kind=-1) == 3
    assert f(kind=0, index=-1) == 3 and f(kind=0, index=8) == 3
    for name in ("policy", "deltas", "gated", "sim", "sim_thr", "real_thr", "returns"):
        assert f(**{name: None}) == 1, name
    assert f(p=bad_n) == 2 and f(p=bad_l) == 4


def test_batch_refuses_what_it_cannot_run_before_touching_the_gpu():
    real = sw.SwimmerEnv("RealWorld", n=3)
    sim = sw.SwimmerEnv("Simulator", n=3, l_i=1.1)
    cost = sw.safe_ars.MaxAbsThetaDot()
    with pytest.raises(TypeError, match="Basic_ARS / Safe_ARS"):
        sw.safe_ars.ARSBatch(real, [1, 2], True, lambda x: abs(x[3]), 1.0, 0.5, sim)
    with pytest.raises(ValueError, match="seed"):
        sw.safe_ars.ARSBatch(real, [], True, cost, 1.0, 0.5, sim)
    with pytest.raises(ValueError, match="gated"):
        sw.safe_ars.ARSBatch(real, [1, 2], [True], cost, 1.0, 0.5, sim)
    with pytest.raises(ValueError, match="real_thresh"):
        sw.safe_ars.ARSBatch(real, [1, 2], True, cost, [1.0, 1.0, 1.0], 0.5, sim)
    with pytest.raises(ValueError, match="sim_envs"):
        sw.safe_ars.ARSBatch(real, [1, 2], True, cost, 1.0, 0.5, [sim])
    with pytest.raises(ValueError, match="gated agents need"):
        sw.safe_ars.ARSBatch(real, [1, 2], [False, True], cost, 1.0)
    with pytest.raises(ValueError, match=r"sim_envs\[1\]"):
        sw.safe_ars.ARSBatch(real, [1, 2], True, cost, 1.0, 0.5, [sim, sw.SwimmerEnv("Simulator", n=4)])
    # scalars broadcast; an all-basic batch needs no simulator
    batch = sw.safe_ars.ARSBatch(real, [1, 2], False, cost, 1.0)
    assert batch.gated.tolist() == [False, False] and batch.real_thresh.tolist() == [1.0, 1.0]
    assert batch.policy.shape == (2, 2, 8)
    with pytest.raises(ValueError, match="costs"):
        batch.train(1, 1, 1, 0.02, 0.5, 10, costs="some")
