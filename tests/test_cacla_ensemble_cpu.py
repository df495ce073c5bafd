"""CACLA gated on an ensemble of simulators without a GPU: the entry point's declaration, binding and argument checks,
the wrapper's parameter names, the classes' constructor errors, the NumPy restatement (tests/cacla_ensemble_oracle.py)
against the single-simulator one, and the soundness of the parity cases the GPU tests run (tests/cacla_ensemble_cases.py):
every decision at least 1e-6 from its edge, at least 4 admitted and 4 refused steps, and a mask that a kernel asking
only member 0 would not produce."""
import ctypes
import os

import numpy as np
import pytest
import torch

import swimmer_amd as sw
from conftest import ROOT
from swimmer_amd import cacla
from swimmer_amd.ars import ensemble as ens
from swimmer_amd.ars.parameters import EnvParam
from swimmer_amd.cacla import safe_kernels
from swimmer_amd.safe_ars import AbsObs, MaxAbsThetaDot

import cacla_ensemble_cases as cases
import cacla_ensemble_oracle as oracle_ens
import cacla_oracle
import cacla_safe_oracle as oracle_se
import test_cacla_safe_gpu as single

HEADER = os.path.join(ROOT, "include", "swimmer_hip.h")
NAME = "sw_cacla_safe_ensemble_run_f64"


def test_entry_point_is_declared_exported_and_bound():
    src = open(HEADER).read()
    assert ("int sw_cacla_safe_ensemble_run_f64(const sw_params *real, int64_t n_agent, int32_t n_member, "
            "int32_t n_iter,") in src
    assert "#define SW_ABI_VERSION 3\n" in src and sw._lib.ABI_VERSION == 3
    assert NAME in sw._lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(sw._lib.library_path()), NAME)
    lib = sw._lib.load()
    assert lib.sw_abi_version() == 3
    assert len(getattr(lib, NAME).argtypes) == 25
    assert "swimmer_cacla_ensemble.hip" in sw._build.SOURCES
    assert not hasattr(sw.kernels, "cacla_safe_ensemble_run") and callable(safe_kernels.cacla_safe_ensemble_run)
    assert cacla.swimmer_experiment.safe_compare_ensemble


# of the 17 pointers from gamma on: 11 admitted_rec, 12 worst_rec, 13 member_refusals and 16 status may be NULL
REQUIRED = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15)
OPTIONAL = (11, 12, 13, 16)


def test_entry_point_validates_without_gpu():
    fn = getattr(sw._lib.load(), NAME)
    ok = sw.SwParams.make(3)
    dev = ctypes.c_void_p(8)          # never dereferenced: validation comes first

    def call(p, n_agent=5, n_member=5, n_iter=16, t_begin=0, kind=sw._lib.COST_MAX_ABS_THETADOT, index=0,
             missing=()):
        ptrs = [None if i in missing else dev for i in range(17)]
        return fn(ctypes.byref(p) if p is not None else None, n_agent, n_member, n_iter, t_begin, *ptrs[:7], kind,
                  index, *ptrs[7:], None)
    assert call(None) == 1
    for missing in REQUIRED:
        assert call(ok, missing=(missing,)) == 1, missing
    assert call(ok, n_member=0) == 3
    assert call(ok, n_member=-1) == 3
    assert call(ok, n_member=65) == 3
    assert call(ok, n_member=64, n_iter=0) == 0                         # a full wave of members is accepted
    assert call(ok, n_member=1, n_iter=0) == 0
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
    assert call(ok, n_iter=0, missing=OPTIONAL) == 0                    # the optional four, absent together ...
    for missing in OPTIONAL:
        assert call(ok, n_iter=0, missing=(missing,)) == 0, missing     # ... and one by one


def _arguments(A=2, E=4, n_iter=5, n=3):
    p = sw.SwParams.make(n)
    f = lambda *shape: torch.zeros(shape, dtype=torch.float64)       # noqa: E731
    i = lambda *shape: torch.zeros(shape, dtype=torch.int32)         # noqa: E731
    return p, dict(gamma=f(A), alpha=f(A), noise=f(A, n_iter, p.m), gated=i(A), sims=f(A, E, 3), sim_thresh=f(A),
                   real_thresh=f(A), weights=f(A, n, cacla.net_doubles(n)), state=f(A, p.d), last_reward=f(A),
                   counters=i(A, 3), first_refused=i(A), rewards=f(A, n_iter), admitted_rec=i(A, n_iter),
                   worst_rec=f(A, n_iter), member_refusals=i(A, E), status=i(A))


_f64, _i32 = torch.float64, torch.int32
BAD = [("alpha", torch.zeros(3, dtype=_f64)), ("noise", torch.zeros((2, 5, 3), dtype=_f64)),
       ("gated", torch.zeros(2, dtype=_f64)), ("sims", torch.zeros((2, 3), dtype=_f64)),            # [A, 3]
       ("sims", torch.zeros((2, 4, 2), dtype=_f64)),                                                 # [A, E, 2]
       ("sims", torch.zeros((2, 0, 3), dtype=_f64)),                                                 # no member
       ("sim_thresh", torch.zeros(2, dtype=torch.float32)), ("real_thresh", None),
       ("weights", torch.zeros((2, 3, 10), dtype=_f64)), ("state", torch.zeros((8, 2), dtype=_f64).t()),
       ("last_reward", torch.zeros((2, 1), dtype=_f64)), ("counters", torch.zeros((2, 3), dtype=torch.int64)),
       ("first_refused", torch.zeros(2, dtype=_f64)), ("rewards", torch.zeros((2, 6), dtype=_f64)),
       ("admitted_rec", torch.zeros((2, 5), dtype=_f64)), ("worst_rec", torch.zeros((2, 5), dtype=torch.float32)),
       ("worst_rec", torch.zeros((2, 6), dtype=_f64)), ("member_refusals", torch.zeros((2, 5), dtype=_i32)),   # E + 1
       ("member_refusals", torch.zeros((2, 4), dtype=_f64)), ("status", torch.zeros(3, dtype=_i32))]


@pytest.mark.parametrize("k", range(len(BAD)), ids=[f"{k}-{name}" for k, (name, _) in enumerate(BAD)])
def test_the_wrapper_names_the_bad_parameter(monkeypatch, k):
    """The checks run on CPU tensors here: the GPU requirement is taken out, and the foreign call is never reached."""
    monkeypatch.setattr(safe_kernels, "require_gpu", lambda: None)
    monkeypatch.setattr(safe_kernels, "_gpu", lambda t, name, ndim: (torch.device("cpu"), name))
    name, bad = BAD[k]
    p, kw = _arguments()
    kw[name] = bad
    with pytest.raises(sw.SwimmerHipError, match=rf"^{name}: expected a contiguous .* as gamma, got "):
        safe_kernels.cacla_safe_ensemble_run(p, 5, 0, cost_kind=1, cost_index=0, **kw)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal is what a machine without a GPU sees")
def test_without_a_gpu_the_wrapper_says_that_there_is_no_cpu_fallback():
    p, kw = _arguments()
    with pytest.raises(sw.SwimmerHipError, match="no CPU fallback"):
        safe_kernels.cacla_safe_ensemble_run(p, 5, 0, cost_kind=1, cost_index=0, **kw)


def _param(n=3, h=1e-3, l_i=1.02):
    return EnvParam("member", n, 0, l_i, 0.97, h, 10.3, 0.0)


def test_constructor_errors():
    env, cost = sw.SwimmerEnv(n=3), MaxAbsThetaDot()
    good = [_param(), _param(l_i=1.03)]
    with pytest.raises(ValueError, match="not both"):
        cacla.CACLA_SE_agent(0.9, 0.01, 1.0, sw.SwimmerEnv(n=3), cost, 0.3, 0.2, sim_ensemble=good)
    with pytest.raises(ValueError, match="at least one simulator"):
        cacla.CACLA_SE_agent(0.9, 0.01, 1.0, None, cost, 0.3, 0.2, sim_ensemble=[])
    with pytest.raises(ValueError, match="at most 64"):
        cacla.CACLA_SE_agent(0.9, 0.01, 1.0, None, cost, 0.3, 0.2, sim_ensemble=[_param()] * 65)
    with pytest.raises(TypeError, match="NativeCost"):
        cacla.CACLA_SE_agent(0.9, 0.01, 1.0, None, abs, 0.3, 0.2, sim_ensemble=good)
    assert cacla.CACLA_SE_agent(0.9, 0.01, 1.0, None, cost, 0.3, 0.2, sim_ensemble=[_param()] * 64)
    # a None simulator threshold is the real threshold itself
    assert cacla.CACLA_SE_agent(0.9, 0.01, 1.0, None, cost, 0.3, None, sim_ensemble=good).sim_threshold == 0.3
    assert cacla.CACLA_SE_agent(0.9, 0.01, 1.0, None, cost, 0.3, 0.2, sim_ensemble=good).sim_threshold == 0.2
    # a member with another n / h / direction: refused by run() before anything is drawn or launched
    for other in (_param(n=4), _param(h=2e-3), sw.SwimmerEnv(n=3, direction=[0.0, 1.0])):
        agent = cacla.CACLA_SE_agent(0.9, 0.01, 1.0, None, cost, 0.3, 0.2, sim_ensemble=[_param(), other])
        with pytest.raises(ValueError, match=r"sim_ensemble\[1\] must have the n, h and direction of env"):
            agent.run(env, 10)
        with pytest.raises(ValueError, match=r"sim_ensemble\[1\] must have the n, h and direction of env"):
            cacla.swimmer_experiment.safe_compare_ensemble(env, [_param(), other], 0.9, 0.01, 1.0, [0], cost, 0.3, 10)
        with pytest.raises(ValueError, match=r"sim_ensembles\[0\]\[1\] must have the n, h and direction of env"):
            cacla.CACLA_SE_Batch(env, [0.9], [0.01], [1.0], [0], None, [0.2], [0.3], cost,
                                 sim_ensembles=[[_param(), other]])
    rows = [(1.0, 1.0, 10.0), (1.02, 0.97, 10.3)]
    with pytest.raises(ValueError, match="same number of members"):                      # ragged
        cacla.CACLA_SE_Batch(env, [0.9] * 2, [0.01] * 2, [1.0] * 2, [0, 1], None, [0.2] * 2, [0.3] * 2, cost,
                             sim_ensembles=[rows, rows[:1]])
    with pytest.raises(ValueError, match="same number of members"):
        cacla.CACLA_SE_Batch(env, [0.9] * 2, [0.01] * 2, [1.0] * 2, [0, 1], None, [0.2] * 2, [0.3] * 2, cost,
                             sim_ensembles=[good, good[:1]])
    with pytest.raises(ValueError, match="not both"):
        cacla.CACLA_SE_Batch(env, [0.9], [0.01], [1.0], [0], [rows[0]], [0.2], [0.3], cost, sim_ensembles=[rows])
    with pytest.raises(ValueError, match="at least one simulator"):
        cacla.CACLA_SE_Batch(env, [0.9], [0.01], [1.0], [0], None, [0.2], [0.3], cost, sim_ensembles=[[]])
    with pytest.raises(ValueError, match="at most 64"):
        cacla.CACLA_SE_Batch(env, [0.9], [0.01], [1.0], [0], None, [0.2], [0.3], cost, sim_ensembles=[rows * 33])
    with pytest.raises(ValueError, match="same length"):                                 # one ensemble, two agents
        cacla.CACLA_SE_Batch(env, [0.9] * 2, [0.01] * 2, [1.0] * 2, [0, 1], None, [0.2] * 2, [0.3] * 2, cost,
                             sim_ensembles=[rows])
    batch = cacla.CACLA_SE_Batch(env, [0.9] * 2, [0.01] * 2, [1.0] * 2, [0, 1], None, None, [0.3, 0.4], AbsObs(3),
                                 sim_ensembles=[rows, good])
    assert batch.sims.shape == (2, 2, 3) and batch.sim_thresholds.tolist() == [0.3, 0.4]
    assert np.array_equal(batch.sims[1], ens.sim_rows(good))
    with pytest.raises(ValueError, match="at least one seed"):
        cacla.swimmer_experiment.safe_compare_ensemble(env, good, 0.9, 0.01, 1.0, [], cost, 0.3, 10)


# ---- the oracle --------------------------------------------------------------------------------------------------
SAME = ("rewards", "admitted", "weights", "state")


@pytest.mark.parametrize("n", (2, 3, 6))
@pytest.mark.parametrize("E", (1, 5))
def test_the_oracle_in_copies_of_one_simulator_is_the_single_oracle_exactly(n, E):
    rs = np.random.RandomState(n)
    w = rs.uniform(-0.3, 0.3, (n, cacla_oracle.net_doubles(n)))
    noise = rs.normal(0.0, 5.0, (40, n - 1))
    one = oracle_se.run(n, 0.9, 0.05, w, noise, oracle_se.max_abs_thetadot, single.SIM, 0.05, 0.04)
    got = oracle_ens.run(n, 0.9, 0.05, w, noise, oracle_ens.max_abs_thetadot, [single.SIM] * E, 0.05, 0.04)
    assert 0 < one["counters"][0] < 40                     # the gate does refuse, and does admit
    for key in SAME:
        assert np.array_equal(got[key], one[key], equal_nan=True), key
    for key in ("counters", "first_refused", "min_sim_margin", "min_real_margin", "min_td"):
        assert got[key] == one[key], key
    assert got["member_refusals"].tolist() == [40 - one["counters"][0]] * E and not got["bad_member"]
    assert np.array_equal(got["worst"] <= 0.05, one["admitted"]) and not np.isnan(got["worst"]).any()
    free = oracle_ens.run(n, 0.9, 0.05, w, noise, oracle_ens.max_abs_thetadot, [single.SIM] * E, 0.05, 0.04, gated=False)
    plain = oracle_se.run(n, 0.9, 0.05, w, noise, oracle_se.max_abs_thetadot, single.SIM, 0.05, 0.04, gated=False)
    for key in SAME:
        assert np.array_equal(free[key], plain[key], equal_nan=True), key
    assert np.isnan(free["worst"]).all() and not free["member_refusals"].any()


def test_the_oracle_refuses_on_nan_on_a_bad_member_and_keeps_everything():
    n = 3
    rs = np.random.RandomState(3)
    w = rs.uniform(-0.3, 0.3, (n, cacla_oracle.net_doubles(n)))
    noise = rs.normal(0.0, 1.0, (10, n - 1))
    sims = [single.SIM, (1.0, 1.0, 10.0), (-1.0, 0.97, 10.3)]
    for rows, thr, bad, refusals in ((sims[:2], np.nan, False, [10, 10]), (sims, np.inf, True, [0, 0, 10])):
        got = oracle_ens.run(n, 0.9, 0.05, w, noise, oracle_ens.abs_obs(3), rows, thr, 0.1)
        assert np.isnan(got["rewards"]).all() and not got["admitted"].any() and got["first_refused"] == 0
        assert got["counters"] == (0, 0, 0) and np.array_equal(got["weights"], w)
        assert got["bad_member"] == bad and got["member_refusals"].tolist() == refusals
        assert (got["worst"] == np.inf).all() if bad else np.isfinite(got["worst"]).all()


# ---- the parity cases are sound ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(cases.CASES))
def test_a_parity_case_is_sound(tag):
    """Not a measurement: a case whose decisions are not all 1e-6 from their edges, or whose mask does not hold four
    steps of each kind, or in which member 0 alone would have given the ensemble's mask, fails here, without a GPU."""
    o = cases.want(tag)
    adm = o["admitted"]
    by_member_0 = int((o["member_in"][:, 0] & ~adm).sum())     # member 0 admits, another member refuses
    print(tag, "admitted", int(adm.sum()), "of", len(adm), "margins (sim, real, temp_diff)",
          o["min_sim_margin"], o["min_real_margin"], o["min_td"], "step 0", bool(adm[0]),
          "member 0 admits, ensemble refuses", by_member_0, "member refusals", o["member_refusals"].tolist(),
          "counters", o["counters"])
    assert min(o["min_sim_margin"], o["min_real_margin"], o["min_td"]) >= 1e-6, o
    assert adm.sum() >= 4 and (~adm).sum() >= 4, adm.sum()
    assert by_member_0 >= 1
    assert not o["bad_member"] and o["member_refusals"].shape == (cases.CASES[tag][1],)
    assert np.array_equal(o["worst"] <= cases.inputs(tag)[4], adm)


def test_the_parity_cases_cover_what_they_are_meant_to():
    """Over the cases: a refusal at step 0, an admitted step 0, a refusal at step 63 with an admission at 64 (the
    block boundary), actor updates, counted violations with real_thresh below sim_thresh, a member other than member 0
    that binds, and the two wrap sizes (64 is no multiple of 7; a full wave of 64) at one and two hidden units per lane."""
    runs = {tag: cases.want(tag) for tag in cases.CASES}
    assert any(not o["admitted"][0] and o["first_refused"] == 0 for o in runs.values())
    assert any(o["admitted"][0] for o in runs.values())
    for tag in ("n3", "n3_abs3"):
        assert not runs[tag]["admitted"][63] and runs[tag]["admitted"][64]
    assert runs["n5"]["counters"][2] > 0 and runs["n6"]["counters"][2] > 0
    assert single.CASES["n8"][4] < single.CASES["n8"][3] and runs["n8"]["counters"][1] > 0
    assert int(np.argmax(runs["n3"]["member_refusals"])) != 0
    assert {cases.CASES[t][1] for t in runs} == {5, 7, 64}
    for E in (7, 64):
        assert {cases.inputs(t)[0] for t in runs if cases.CASES[t][1] == E} == {3, 6}
    # the members are distinct simulators, member 0 the single-simulator cases' own
    rows = cases.inputs("n3_e64")[6]
    assert len({tuple(r) for r in rows}) == 64 and tuple(rows[0]) == single.SIM
