"""CACLA on LQR without a GPU: the NumPy restatement (tests/lqr_oracle.py) against the reference's own runs
(tests/golden/lqr.npz), the host side's random streams, the environment classes, window_convolution, the recognition
of costs, and the C entry point's declaration and argument checks."""
import ctypes
import os

import numpy as np
import pytest

import swimmer_amd as sw
from conftest import GOLDEN, ROOT
from swimmer_amd import cacla
from swimmer_amd.cacla import cacla_safe_agent, lqr
from swimmer_amd.envs.gym_lqr import lqr_env

import lqr_oracle

HEADER = os.path.join(ROOT, "include", "swimmer_hip.h")
CASES = tuple(lqr_oracle.CASES)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "lqr.npz"), allow_pickle=False)


@pytest.mark.parametrize("tag", CASES)
def test_oracle_reproduces_the_reference(gold, tag):
    """Every case, every step, 1e-12 absolute; shapes (the short and the empty arrays included) and counters exact."""
    case = lqr_oracle.CASES[tag]
    res = lqr_oracle.run_case(case, lqr_env, gold[f"{tag}_x0"], gold[f"{tag}_noise"])
    got = lqr_oracle.reference_arrays(res)
    err = {}
    for name, g in zip(("states", "actions", "rewards"), got):
        want = gold[f"{tag}_{name}"]
        assert g.shape == want.shape, (name, g.shape, want.shape)
        err[name] = float(np.abs(g - want).max()) if want.size else 0.0
    for name in ("F", "V", "state"):
        err[name] = float(np.abs(res[name] - gold[f"{tag}_{name}"]).max())
    print(f"case {tag}: {err}")
    assert max(err.values()) <= 1e-12, err
    assert [res["admitted"], res["violations"], res["actor_updates"]] == gold[f"{tag}_counters"].tolist()
    assert res["min_td"] >= 1e-6 and res["min_gap"] >= 1e-6


def test_the_table_of_cases_is_the_goldens(gold):
    for tag, case in lqr_oracle.CASES.items():
        seed, steps, gamma, alpha, sigma, l = gold[f"{tag}_hyper"]
        assert (seed, steps, gamma, alpha, sigma, l) == (case["seed"], case["steps"], case["gamma"], case["alpha"],
                                                          case["sigma"], case.get("l", 0.0))
    assert gold["S8_states"].shape == (0,) and gold["L32_states"].shape == (223, 2)
    assert gold["V0_counters"].tolist() == [172, 52, 6] and gold["V0_rewards"].shape == (253,)


@pytest.mark.parametrize("tag", CASES)
def test_host_streams_are_the_references(gold, tag):
    """x0 and the noise in chunks of odd size from NumPy's global stream and from a RandomState: equal to what the
    reference's run drew, and the stream is left where the reference leaves it."""
    case = lqr_oracle.CASES[tag]
    x0, noise = gold[f"{tag}_x0"], gold[f"{tag}_noise"]
    T, na = noise.shape
    cov, zeros = case["sigma"] * np.identity(na), np.zeros(na)
    np.random.seed(case["seed"])
    assert np.array_equal(np.random.rand(len(x0)), x0)
    drawn = np.concatenate([np.random.multivariate_normal(zeros, cov, size=k) for k in (37, 101, T - 138)])
    assert np.array_equal(drawn, noise)
    assert np.random.standard_normal() == gold[f"{tag}_next_normal"]
    before = np.random.get_state()[1].copy()
    rs = np.random.RandomState(case["seed"])
    assert np.array_equal(rs.rand(len(x0)), x0)
    assert np.array_equal(np.concatenate([rs.multivariate_normal(zeros, cov, size=k) for k in (T - 5, 5)]), noise)
    assert rs.standard_normal() == gold[f"{tag}_next_normal"]
    assert np.array_equal(np.random.get_state()[1], before)


def _envs():
    return {"LinearQuadReg": lqr_oracle.make_env(lqr_env, "p13"),
            "EasyParamLinearQuadReg": lqr_env.EasyParamLinearQuadReg(0.9),
            "BoundedEasyLinearQuadReg": lqr_env.BoundedEasyLinearQuadReg(0.95, 1.0, 0.5),
            "BoundedActionEasyLinearQuadReg": lqr_env.BoundedActionEasyLinearQuadReg(0.95, 1.0),
            "EasyAffineQuadReg": lqr_env.EasyAffineQuadReg(0.99)}


@pytest.mark.parametrize("name", lqr_oracle.ENV_CLASSES)
def test_environments_match_the_references_transitions(gold, name):
    env = _envs()[name]
    env.set_state(gold[f"env_{name}_s0"].copy())
    m = lqr_oracle.model(env)
    clipped = 0
    for t, u in enumerate(gold[f"env_{name}_u"]):
        before = np.array(env.state)
        obs, rew, done, info = env.step(u.copy())
        assert done is False and obs is env.state
        assert np.abs(obs - gold[f"env_{name}_states"][t]).max() <= 1e-15
        assert abs(rew - gold[f"env_{name}_rewards"][t]) <= 1e-15
        assert np.abs(info["action"] - gold[f"env_{name}_actions"][t]).max() <= 1e-15
        sn, a = lqr_oracle.env_step(m, before, u)                    # the oracle's step is the same map
        assert np.abs(sn - obs).max() <= 1e-15 and np.abs(a - info["action"]).max() <= 1e-15
        clipped += int(not np.array_equal(info["action"], u))
    assert (clipped > 0) == name.startswith("Bounded")
    assert env.observation_space.shape == (len(gold[f"env_{name}_s0"]),)
    assert env.action_space.shape == (gold[f"env_{name}_u"].shape[1],)
    if name != "LinearQuadReg":
        assert env.op_norm_der_A == 1 and env.op_norm_der_B == 1
    A, B, C, max_s, max_a, Q, R = lqr_env.model_of(env)
    assert (max_s, max_a) == {"BoundedEasyLinearQuadReg": (1.0, 0.5),
                              "BoundedActionEasyLinearQuadReg": (0.0, 1.0)}.get(name, (0.0, 0.0))
    assert np.array_equal(C, [0.099, 0.0]) if name == "EasyAffineQuadReg" else not C.any()
    np.random.seed(5)
    want = np.random.rand(A.shape[0])
    np.random.seed(5)
    assert np.array_equal(env.reset(), want) and env.state is not None


def test_window_convolution_is_exactly_the_references(gold):
    got = cacla.window_convolution(gold["window_a"], int(gold["window_H"]))
    assert got.shape == gold["window_out"].shape == (250,)
    assert np.array_equal(got, gold["window_out"])
    assert cacla.window_convolution(np.arange(5.0), 5).shape == (0,)
    assert cacla.window_convolution(np.array([]), 3).shape == (0,)


def test_cost_recognition():
    K = sw.kernels
    for ord_, code in ((np.inf, K.LQR_COST_INF), (2, K.LQR_COST_2), (1, K.LQR_COST_1)):
        for ns in (2, 3, 4):
            assert lqr.cost_code(lambda x, o=ord_: np.linalg.norm(x, o), ns) == code
            assert lqr.cost_code(cacla.norm_cost(ord_), ns) == code
        x = np.array([0.5, -2.0, 1.0])
        assert cacla.norm_cost(ord_)(x) == np.linalg.norm(x, ord_)
    assert lqr.cost_code(lambda x: np.linalg.norm(x), 2) == K.LQR_COST_2
    assert lqr.cost_code(lambda x: np.abs(x).max(), 2) == K.LQR_COST_INF
    for bad in (lambda x: x[0] ** 2, lambda x: 2 * np.linalg.norm(x, np.inf), lambda x: abs(x[0]), "inf", None,
                lambda x: x, lambda: 0.0):
        with pytest.raises(TypeError, match="inf-, 2- and 1-norm"):
            lqr.cost_code(bad, 2)
    with pytest.raises(TypeError):
        cacla.norm_cost(3)
    c = cacla_safe_agent.Constraint(cacla.norm_cost(np.inf), 1.0, 1)
    assert c.satisfied(np.array([1.0, -0.5])) and not c.satisfied(np.array([1.0, -1.5]))
    with pytest.raises(TypeError):                                  # refused when the agent is made, not in run()
        cacla_safe_agent.CACLA_LQR_SE_agent(lqr_env.EasyParamLinearQuadReg(1.0), lqr_env.EasyParamLinearQuadReg(0.9),
                                            0.1, cacla_safe_agent.Constraint(lambda x: x[0], 1.0, 1))


def test_agents_are_built_as_the_references(gold):
    """Constructors, attributes and the fixed thresholds, without a run."""
    for tag, case in lqr_oracle.CASES.items():
        agent, real, sim = lqr_oracle.build(case, lqr_env, cacla.CACLA_LQR_agent, cacla_safe_agent)
        ns, na = np.asarray(real.A).shape[1], np.asarray(real.B).shape[1]
        assert agent.F.shape == (na, ns) and not agent.F.any() and agent.V.shape == (ns,) and agent.env is real
        if case["kind"] == "bounded":
            eps = lqr_oracle.epsilon_of(case)
            want = case["l"] - eps * 1 * (np.sqrt(2) * real.max_s + np.sqrt(1) * real.max_a)
            assert agent.sim_threshold == want
            assert lqr.fixed_threshold("bounded", real, sim, eps, agent.constraint) == want
        if case["kind"] == "affine":
            assert agent.sim_threshold == case["l"] - lqr_oracle.epsilon_of(case) * 1 * np.linalg.norm([0.1, 0])
    fix = cacla_safe_agent.CACLA_LQR_SE_fix(lqr_env.EasyParamLinearQuadReg(1.0), lqr_env.EasyParamLinearQuadReg(0.9),
                                            0.1, cacla_safe_agent.Constraint(cacla.norm_cost(2), 2.0, 1.5))
    fix.set_simulator_threshold(3.0)
    assert fix.sim_threshold == 2.0 - 0.1 * 1.5 * 3.0
    assert fix.compute_sim_threshold(1.5, 0.1, np.array([3.0, 4.0]), np.array([2.0])) == 2.0 - 0.1 * 1.5 * 7.0
    a = cacla.CACLA_LQR_agent(lqr_oracle.make_env(lqr_env, "p13"))
    a.F[...] = np.arange(6.0).reshape(2, 3)
    a.V[...] = [1.0, 2.0, 3.0]
    s = np.array([1.0, -1.0, 2.0])
    assert np.array_equal(a.forward_action_FA(s), a.F @ s) and a.forward_value_FA(s) == 1.0 + 2.0 + 12.0


def test_parameter_block_layout():
    """pack_params is the header's SW_LQR_PARAM_DOUBLES block, in its order."""
    src = open(HEADER).read()
    assert "#define SW_LQR_MODEL_DOUBLES(ns, na) ((ns) * (ns) + (ns) * (na) + (ns) + 2)" in src
    assert "#define SW_LQR_PARAM_DOUBLES(ns, na) (2 * SW_LQR_MODEL_DOUBLES(ns, na) + (ns) * (ns) + (na) * (na) + 7)" in src
    real = lqr_env.BoundedEasyLinearQuadReg(0.95, 2.0, 1.0)
    sim = lqr_env.EasyAffineQuadReg(0.5)
    col = lqr.pack_params(lqr_env.model_of(real), lqr_env.model_of(sim), 0.9, 0.01, 1.5, 0.05, 1.0, 1.0, 1.25)
    assert len(col) == sw.kernels.lqr_param_doubles(2, 1) == 2 * sw.kernels.lqr_model_doubles(2, 1) + 4 + 1 + 7 == 32
    assert col.tolist() == [0, .95, .95, 0, 0, .95, 0, 0, 2.0, 1.0,   0, 1, 1, 0, 0, 1, 0.05, 0, 0, 0,
                            1, 0, 0, 1, 1,   0.9, 0.01, 1.5, 0.05, 1.0, 1.0, 1.25]
    for ns in range(1, 5):
        for na in range(1, 3):
            assert sw.kernels.lqr_param_doubles(ns, na) == 2 * (ns * ns + ns * na + ns + 2) + ns * ns + na * na + 7


def test_entry_point_is_declared_and_exported():
    src = open(HEADER).read()
    assert "int sw_lqr_cacla_run_f64(int32_t ns, int32_t na, int64_t n_agent, int32_t n_iter, int32_t safe," in src
    assert "sw_lqr_cacla_run_f64" in sw._lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(sw._lib.library_path()), "sw_lqr_cacla_run_f64")
    assert sw._lib.load().sw_abi_version() == 3 and "#define SW_ABI_VERSION 3" in src
    assert "swimmer_lqr.hip" in sw._build.SOURCES
    for name, value in (("SW_LQR_MAX_STATE", sw.kernels.LQR_MAX_STATE), ("SW_LQR_MAX_ACTION", sw.kernels.LQR_MAX_ACTION),
                        ("SW_LQR_THRESHOLD_STEP", sw.kernels.LQR_THRESHOLD_STEP),
                        ("SW_LQR_THRESHOLD_FIXED", sw.kernels.LQR_THRESHOLD_FIXED),
                        ("SW_LQR_COST_INF", sw.kernels.LQR_COST_INF), ("SW_LQR_COST_2", sw.kernels.LQR_COST_2),
                        ("SW_LQR_COST_1", sw.kernels.LQR_COST_1), ("SW_LQR_REFUSED", sw.kernels.LQR_REFUSED),
                        ("SW_LQR_ADMITTED", sw.kernels.LQR_ADMITTED), ("SW_LQR_NOTHING_YET", sw.kernels.LQR_NOTHING_YET)):
        assert f"#define {name} {value}" in src, name


def test_entry_point_validates_without_gpu():
    fn = sw._lib.load().sw_lqr_cacla_run_f64
    dev = ctypes.c_void_p(8)          # never dereferenced: validation comes first

    def call(ns=2, na=1, n_agent=5, n_iter=16, safe=1, threshold=0, cost=0, missing=None):
        # params noise F V state last counters status | the four records may be NULL
        ptrs = [None if i == missing else dev for i in range(8)]
        return fn(ns, na, n_agent, n_iter, safe, threshold, cost, *ptrs, None, None, None, None, None)
    for missing in range(8):
        assert call(missing=missing) == 1
    assert call(n_agent=0) == 3
    assert call(n_agent=-4) == 3
    assert call(n_agent=2 ** 31) == 3
    assert call(n_iter=-1) == 3
    for ns, na in ((0, 1), (5, 1), (2, 3), (2, 0), (-1, 1)):
        assert call(ns=ns, na=na) == 3
    assert call(safe=2) == 4 and call(safe=-1) == 4
    assert call(threshold=2) == 4
    assert call(cost=3) == 4 and call(cost=-1) == 4
    assert call(missing=0, n_agent=0) == 1                              # NULL is reported first
    for ns in (1, 4):
        for na in (1, 2):
            assert call(ns=ns, na=na, n_iter=0) == 0                    # nothing to do, nothing written
    assert call(n_iter=0, safe=0, threshold=1, cost=2) == 0
