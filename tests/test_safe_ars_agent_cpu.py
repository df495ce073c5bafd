"""ARSAgent(safe=True) pieces that need no GPU: the approximation branch and the simulator threshold against the
reference's fixtures, the construction-time argument errors, the CPU restatement of the safe iteration against
the reference (tests/golden/safe_agent.npz, make_safe_agent_golden.py), and the gate's C ABI entry."""
import os
import warnings

import numpy as np
import pytest

import swimmer_amd as sw
from swimmer_amd import _lib
from swimmer_amd.ars import ars_agent
from swimmer_amd.ars.parameters import Threshold
from conftest import GOLDEN, ROOT
from safe_agent_oracle import SafeArsOracle

CASES = "abcdefgh"
DB = os.path.join(GOLDEN, "safe_agent_db.npz")


def _fixture():
    return np.load(os.path.join(GOLDEN, "safe_agent.npz"), allow_pickle=False)


def _params(g, tag):
    n, V1, N, b, H, seed, iters, gseed, exact = (int(x) for x in g[tag + "_cfg"])
    l_i, m_i, k, h, eps, alpha, nu, thr, K, A, B = g[tag + "_phys"]
    ep = sw.EnvParam("LeonSwimmer-RealWorld", n=n, H=H, l_i=l_i, m_i=m_i, h=h, k=k, epsilon=eps)
    ap = sw.ARSParam("SafeGolden", V1=bool(V1), n_iter=iters - 1, H=H, N=N, b=b, alpha=alpha, nu=nu,
                     safe=True, threshold=thr, initial_w="Zero")
    return ep, ap, Threshold(K, A, B), dict(seed=seed, gseed=gseed, exact=bool(exact), eps=eps)


@pytest.mark.parametrize("tag", CASES)
def test_estimation_and_simulator_threshold_match_the_reference(tag):
    g = _fixture()
    ep, ap, thresh, c = _params(g, tag)
    np.random.seed(c["gseed"])
    est = ep if c["exact"] else ars_agent.approximate_env_param(ep, c["eps"])
    assert (est is ep) and (c["exact"] or est.name == "LeonSwimmer-Simulator")
    assert np.array_equal([est.l_i, est.m_i, est.k, est.h], g[tag + "_estimated"])
    assert ars_agent.simulator_threshold(ap, ep, thresh) == g[tag + "_sim_threshold"]


def _safe_param(**kw):
    return sw.ARSParam("Safe", V1=True, n_iter=1, H=10, N=2, b=2, alpha=0.01, nu=0.01, safe=True,
                       threshold=0.0, initial_w="Zero", **kw)


def _env():
    return sw.EnvParam("RealWorld", n=3, H=10, l_i=1.0, m_i=1.0, h=1e-3, k=10.0, epsilon=0.01)


def test_safe_without_sim_thresh_raises_value_error():
    with pytest.raises(ValueError, match="sim_thresh"):
        sw.ARSAgent(_env(), _safe_param(), data_path=DB, seed=0)


def test_safe_without_data_path_raises_value_error():
    with pytest.raises(ValueError, match="data_path"):
        sw.ARSAgent(_env(), _safe_param(), seed=0, sim_thresh=Threshold(1, 0.3, 0.001))


def test_safe_with_several_ranks_raises_not_implemented(monkeypatch):
    monkeypatch.setattr(ars_agent.dist, "is_available", lambda: True)
    monkeypatch.setattr(ars_agent.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(ars_agent.dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(ars_agent.dist, "get_rank", lambda group=None: 0)
    with pytest.raises(NotImplementedError, match="one rank"):
        sw.ARSAgent(_env(), _safe_param(), data_path=DB, seed=0, sim_thresh=Threshold(1, 0.3, 0.001))


def run_oracle(g, tag):
    """The restatement on case `tag`: (oracle, per-iteration returns, curve)."""
    ep, ap, thresh, c = _params(g, tag)
    real = (ep.l_i, ep.m_i, ep.k, ep.h)
    est = g[tag + "_estimated"]
    o = SafeArsOracle(ep.n, real, (est[0], est[1], est[2], est[3]), ap.H, ap.N, ap.b, ap.alpha, ap.nu, ap.V1,
                      ap.threshold, float(g[tag + "_sim_threshold"]), c["seed"], policy0=g[tag + "_w0"])
    per_it = []
    inner = o.iteration

    def recorded():
        r = inner()
        per_it.append(r)
        return r
    o.iteration = recorded
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # np.mean([]) of an all-refused first iteration
        curve = o.training(ap.n_iter)
    return o, per_it, curve


def _close(a, b, tol=1e-9):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan)
    scale = max(1.0, float(np.abs(b[~nan]).max())) if (~nan).any() else 1.0
    assert np.all(np.abs(a[~nan] - b[~nan]) <= tol * scale)


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference(tag):
    g = _fixture()
    o, per_it, curve = run_oracle(g, tag)
    counts = np.array([len(r) for r in per_it])
    assert np.array_equal(counts, g[tag + "_counts"])
    for j, r in enumerate(per_it):
        _close(r, g[tag + "_returns"][j][:len(r)])
    _close(curve, g[tag + "_curve"])
    _close(o.policy, g[tag + "_policy"])
    if tag + "_mean" in g.files:
        _close(o.mean, g[tag + "_mean"])
        _close(o.covariance, g[tag + "_cov"])
    assert o.violations == int(g[tag + "_below"])


def test_fixture_cases_cover_refusals():
    g = _fixture()
    for tag in "abcd":
        refused = np.mean(g[tag + "_counts"] == 0)
        assert 0.3 <= refused <= 0.7, (tag, refused)
    assert np.all(g["e_counts"] == 8) and np.all(g["f_counts"] == 0)
    assert 0.0 < np.mean(g["g_counts"] == 0) < 1.0 and not bool(g["g_cfg"][1])    # row form, V2, partial
    assert int(g["h_below"]) > 0                                                  # violations to count


def test_gate_entry_is_declared_and_exported():
    with open(os.path.join(ROOT, "include", "swimmer_hip.h")) as f:
        header = f.read()
    assert "int sw_ars_gate_f64(const sw_params *sim, int64_t dir_begin, int64_t n_dir, int32_t H," in header
    assert "sw_ars_gate_f64" in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 3
