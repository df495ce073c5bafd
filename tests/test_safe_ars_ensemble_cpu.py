"""Safe ARS rollouts gated on an ensemble of simulators, without a GPU: the entry point's declaration, binding and
argument checks, the wrapper's parameter names, ARSBatch's constructor errors, the NumPy restatement
(tests/safe_ensemble_oracle.py) against the single-simulator one, and the soundness of the cases the GPU tests compare
with the oracle (tests/safe_ensemble_cases.py): refused and unrefused rollouts, a rollout in which only some members
refuse, and every gate decision more than 1e-6 from its edge."""
import ctypes
import os

import numpy as np
import pytest
import torch

import swimmer_amd as sw
from conftest import ROOT
from oracle import safe_ars_oracle as sao
from oracle import swimmer_oracle as so
from swimmer_amd.safe_ars import ensemble_kernels, experiment

import safe_ensemble_cases as cases
import safe_ensemble_oracle as oracle_ens

HEADER = os.path.join(ROOT, "include", "swimmer_hip.h")
NAME = "sw_safe_ars_rollouts_ensemble_f64"
MAX, ABS = sw._lib.COST_MAX_ABS_THETADOT, sw._lib.COST_ABS_OBS


def test_entry_point_is_declared_exported_and_bound():
    src = open(HEADER).read()
    assert ("int sw_safe_ars_rollouts_ensemble_f64(const sw_params *real, int64_t n_agent, int32_t n_member, "
            "int64_t n_dir, int32_t H,") in src
    assert "#define SW_ABI_VERSION 3\n" in src and sw._lib.ABI_VERSION == 3
    assert NAME in sw._lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(sw._lib.library_path()), NAME)
    lib = sw._lib.load()
    assert lib.sw_abi_version() == 3
    assert len(getattr(lib, NAME).argtypes) == 23
    assert "swimmer_safe_ars_ensemble.hip" in sw._build.SOURCES
    assert "swimmer_safe_ars_ensemble.hip" not in sw._build.FAMILIES          # a translation unit of its own
    assert sw.kernels.safe_ars_rollouts_ensemble is ensemble_kernels.safe_ars_rollouts_ensemble
    assert callable(experiment.run_ensemble)


# of the 14 pointers: policy, deltas | gated, sims, sim_thresh, real_thresh | returns are required
REQUIRED = (0, 1, 2, 3, 4, 5, 6)
OPTIONAL = (7, 8, 9, 10, 11, 12, 13)      # cost_trace, cost_max, first_refused, violations, status, worst_max, mask


def test_entry_point_validates_without_gpu():
    fn = getattr(sw._lib.load(), NAME)
    ok = sw.SwParams.make(3)
    dev = ctypes.c_void_p(8)          # never dereferenced: every call below is refused before any HIP call

    def call(p, n_agent=3, n_member=5, n_dir=9, H=5, kind=MAX, index=0, missing=()):
        ptrs = [None if i in missing else dev for i in range(14)]
        return fn(ctypes.byref(p) if p is not None else None, n_agent, n_member, n_dir, H, ptrs[0], ptrs[1], 0.4,
                  *ptrs[2:6], kind, index, *ptrs[6:], None)
    assert call(None) == 1
    for missing in REQUIRED:
        assert call(ok, missing=(missing,)) == 1, missing
    twin = sw.SwParams.make(3, flags=sw._lib.FLAG_MODEL_TWIN)
    assert call(twin) == 4                                              # the last check before the launch ...
    for missing in OPTIONAL:
        assert call(twin, missing=(missing,)) == 4, missing             # ... so an absent optional output got there
    assert call(twin, missing=OPTIONAL) == 4
    for flags in (sw._lib.FLAG_ROLLOUT_LANE, sw._lib.FLAG_ROLLOUT_QUAD):
        assert call(sw.SwParams.make(3, flags=flags), missing=(0,)) == 1    # accepted: the next complaint is the NULL
    assert call(ok, n_member=0) == 3
    assert call(ok, n_member=-1) == 3
    assert call(ok, n_member=65) == 3
    assert call(twin, n_member=64) == 4                                 # a full wave of members is accepted
    assert call(twin, n_member=1) == 4
    assert call(ok, n_agent=0) == 3
    assert call(ok, n_agent=65536) == 3
    assert call(ok, n_dir=0) == 3
    assert call(ok, n_dir=2 ** 23 + 1) == 3
    assert call(ok, H=-1) == 3
    assert call(ok, kind=2) == 3
    assert call(ok, kind=ABS, index=8) == 3                             # d = 8: 0..7
    assert call(ok, kind=ABS, index=-1) == 3
    assert call(twin, kind=MAX, index=99) == 4                          # the index is not read
    # 2^32 threads and more, counted WITH the group: 65535 agents x 2^16 rollouts x 1 lane fit, x 2 lanes do not
    assert call(twin, n_agent=65535, n_member=1, n_dir=2 ** 15) == 4
    assert call(ok, n_agent=65535, n_member=2, n_dir=2 ** 15) == 3
    assert call(ok, n_agent=1024, n_member=33, n_dir=2 ** 15) == 3      # 2^10 x 2^16 groups of 64
    assert call(twin, n_agent=1023, n_member=64, n_dir=2 ** 15) == 4
    assert call(sw.SwParams.make(9)) == 2
    assert call(sw.SwParams.make(3, l_i=-1.0)) == 4


def _arguments(A=2, E=4, N=3, H=5, n=3):
    p = sw.SwParams.make(n)
    f = lambda *shape: torch.zeros(shape, dtype=torch.float64)       # noqa: E731
    i = lambda *shape: torch.zeros(shape, dtype=torch.int32)         # noqa: E731
    return p, dict(policy=f(A, p.m, p.d), deltas=f(A, N, p.m, p.d), gated=i(A), sims=f(A, E, 3), sim_thresh=f(A),
                   real_thresh=f(A), returns=f(A, 2 * N), cost_trace=f(H, A, 2 * N), cost_max=f(A, 2 * N),
                   first_refused=i(A, 2 * N), violations=i(A, 2 * N), status=i(A, 2 * N), worst_max=f(A, 2 * N),
                   refusing_members=torch.zeros((A, 2 * N), dtype=torch.int64))


_f64, _i32, _i64 = torch.float64, torch.int32, torch.int64
BAD = [("sims", torch.zeros((2, 3), dtype=_f64)),                                                    # [A, 3]
       ("sims", torch.zeros((2, 4, 2), dtype=_f64)),                                                 # [A, E, 2]
       ("sims", torch.zeros((3, 4, 3), dtype=_f64)),                                                 # another A
       ("sims", torch.zeros((2, 0, 3), dtype=_f64)),                                                 # E = 0
       ("sims", torch.zeros((2, 4, 3), dtype=torch.float32)), ("sims", None),
       ("sims", torch.zeros((2, 4, 3), dtype=_f64, device="meta")),
       ("sims", torch.zeros((2, 4, 3, 2), dtype=_f64)[..., 0]),
       ("worst_max", torch.zeros((2, 6), dtype=torch.float32)), ("worst_max", torch.zeros((2, 5), dtype=_f64)),
       ("worst_max", torch.zeros((2, 6), dtype=_f64, device="meta")),
       ("refusing_members", torch.zeros((2, 6), dtype=_i32)), ("refusing_members", torch.zeros((2, 6), dtype=_f64)),
       ("refusing_members", torch.zeros((2, 7), dtype=_i64)), ("refusing_members", torch.zeros((6, 2), dtype=_i64).t()),
       ("refusing_members", torch.zeros((2, 6), dtype=_i64, device="meta")),
       ("gated", torch.zeros(2, dtype=_f64)), ("sim_thresh", torch.zeros(3, dtype=_f64)), ("real_thresh", None),
       ("cost_trace", torch.zeros((2, 5, 6), dtype=_f64)), ("status", torch.zeros((2, 6), dtype=_i64))]


@pytest.mark.parametrize("k", range(len(BAD)), ids=[f"{k}-{name}" for k, (name, _) in enumerate(BAD)])
def test_the_wrapper_names_the_bad_parameter(monkeypatch, k):
    """The checks run on CPU tensors here: the GPU requirement is taken out, and the foreign call is never reached."""
    monkeypatch.setattr(ensemble_kernels, "require_gpu", lambda: None)
    monkeypatch.setattr(sw.kernels, "_gpu", lambda t, name, ndim: (torch.device("cpu"), name))
    name, bad = BAD[k]
    p, kw = _arguments()
    kw[name] = bad
    with pytest.raises(sw.SwimmerHipError, match=rf"^{name}: expected a contiguous .* as policy, got "):
        sw.kernels.safe_ars_rollouts_ensemble(p, 5, nu=0.4, cost_kind=MAX, cost_index=0, **kw)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal is what a machine without a GPU sees")
def test_without_a_gpu_the_wrapper_says_that_there_is_no_cpu_fallback():
    p, kw = _arguments()
    with pytest.raises(sw.SwimmerHipError, match="no CPU fallback"):
        sw.kernels.safe_ars_rollouts_ensemble(p, 5, nu=0.4, cost_kind=MAX, cost_index=0, **kw)


def test_batch_constructor_errors():
    real, cost = sw.SwimmerEnv(n=3), sw.safe_ars.MaxAbsThetaDot()
    sim = sw.SwimmerEnv("Simulator", n=3, l_i=1.02, m_i=0.97, k=10.3)
    rows = [(1.0, 1.0, 10.0), (1.02, 0.97, 10.3)]
    make = lambda gated, ens, **kw: sw.safe_ars.ARSBatch(real, [1] * len(gated), gated, cost, 3.0, **kw,     # noqa: E731
                                                         sim_ensembles=ens)
    with pytest.raises(ValueError, match="not both"):
        make([True], [rows], sim_thresh=2.0, sim_envs=sim)
    with pytest.raises(ValueError, match="same number of members"):                      # ragged
        make([True, True], [rows, rows[:1]])
    with pytest.raises(ValueError, match="same number of members"):
        make([True, False, True], [[sim, sim, sim], None, rows])
    with pytest.raises(ValueError, match=r"sim_ensembles\[1\]: a gated agent needs an ensemble"):
        make([False, True], [None, None])
    with pytest.raises(ValueError, match="one entry per agent"):
        make([True, True], [rows])
    with pytest.raises(ValueError, match="1 to 64 simulators"):
        make([True], [[]])
    with pytest.raises(ValueError, match="1 to 64 simulators"):
        make([True], [rows * 33])
    with pytest.raises(ValueError, match=r"sim_ensembles\[0\]\[1\]: n, h and the direction"):
        make([True], [[sim, sw.SwimmerEnv(n=4)]])
    with pytest.raises(ValueError, match="rows"):
        make([True], [[(1.0, 1.0)]])
    # without sim_ensembles the old rule stands
    with pytest.raises(ValueError, match="gated agents need sim_thresh and sim_envs"):
        sw.safe_ars.ARSBatch(real, [1], [True], cost, 3.0)
    # objects and rows mix, an ungated agent's rows are the real swimmer's, a None threshold is the real one
    batch = make([True, False, True], [[sim, rows[0]] * 32, None, rows * 32])
    assert batch.ensemble and batch.sims.shape == (3, 64, 3)
    assert batch.sims[0, :2].tolist() == [[1.02, 0.97, 10.3], [1.0, 1.0, 10.0]]
    assert np.array_equal(batch.sims[1], np.tile([real.l_i, real.m_i, real.k], (64, 1)))
    assert np.array_equal(batch.sims[2], np.array(rows * 32))
    assert batch.sim_thresh.tolist() == [3.0] * 3
    assert make([True, True], [rows, rows], sim_thresh=[2.0, 2.5]).sim_thresh.tolist() == [2.0, 2.5]
    plain = sw.safe_ars.ARSBatch(real, [1], [True], cost, 3.0, 2.0, sim)
    assert not plain.ensemble and plain.sims is None


def test_the_experiments_members():
    theta = np.array([1.01, 0.98, 10.02])
    state = np.random.get_state()
    rows = experiment.ensemble_members(theta, 0.05, 8, ensemble_seed=3)
    assert np.array_equal(np.random.get_state()[1], state[1])               # the global generator is not touched
    assert rows.shape == (8, 3) and np.array_equal(rows[0], theta)
    rs = np.random.RandomState(3)
    for row in rows[1:]:
        g = rs.standard_normal(3)
        assert np.array_equal(row, theta + 0.05 * (g / np.linalg.norm(g, ord=2)))
    assert np.allclose(np.linalg.norm(rows[1:] - theta, axis=1), 0.05, rtol=1e-12, atol=0)
    assert np.array_equal(experiment.ensemble_members(theta, 0.05, 1), theta[None])
    with pytest.raises(ValueError):
        experiment.ensemble_members(theta, 0.05, 0)


# ---- the oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2, 3, 6))
@pytest.mark.parametrize("E", (1, 4))
def test_the_oracle_in_copies_of_one_simulator_is_the_single_oracle_exactly(n, E):
    cost = (ABS, 3, (0.3, 0.4), 0.004)
    c = cases.ensemble_case(n, 3, 1, cost)
    p_real = so.OracleParams.make(n)
    fn = oracle_ens.cost_fn(ABS, 3)
    refused = 0
    for a in (0, 2):
        p_sim = so.OracleParams.make(n, *c["sims"][a, 0])
        for r in range(6):
            pol = c["policy"][a] + (-1.0 if r & 1 else 1.0) * c["nu"] * c["deltas"][a, r >> 1]
            R, states = sao.safe_rollout(p_real, p_sim, fn, c["sim_thresh"][a], pol, 21)
            got = oracle_ens.rollout(p_real, [p_sim] * E, fn, c["sim_thresh"][a], c["real_thresh"][a], pol, 21)
            assert got["R"] == R and np.array_equal(got["states"], states), (a, r)
            assert got["refusing"] == (0 if got["first_refused"] == 21 else (1 << E) - 1)
            assert got["worst_max"] <= c["sim_thresh"][a]
            refused += got["first_refused"] < 21
            free = oracle_ens.rollout(p_real, [], fn, 0.0, c["real_thresh"][a], pol, 21, gated=False)
            R_free, traj = sao.safe_rollout(p_real, p_sim, fn, np.inf, pol, 21)        # a gate that is always open
            assert free["R"] == R_free and np.array_equal(free["states"], traj) and np.isnan(free["worst_max"])
            assert free["first_refused"] == 21 and free["refusing"] == 0
    assert refused > 0                                    # the gate does refuse here


def test_the_rule_refuses_on_nan_and_names_the_members():
    assert oracle_ens.admits([0.1, 0.2, 0.3], 0.3) == (True, 0)
    assert oracle_ens.admits([0.1, 0.31, 0.3], 0.3) == (False, 2)
    assert oracle_ens.admits([np.nan, 0.2, 0.4], 0.3) == (False, 5)
    assert oracle_ens.admits([0.1, 0.2], np.nan) == (False, 3)


# ---- the conditioned cases are sound ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k_cost", (0, 1), ids=("max_abs_thetadot", "abs_obs_3"))
@pytest.mark.parametrize("E", (3, 5))
def test_a_conditioned_case_is_sound(E, k_cost):
    """Not a measurement: a case in which a gated agent has no refused or no unrefused rollout, no rollout where a proper
    subset of the members refuses, or a gate decision within 1e-6 of its threshold fails here, without a GPU."""
    H = 51
    o = cases.want(3, 9, E, k_cost, H)
    for a in (0, 2):
        first, mask = o["first_refused"][a], o["refusing"][a]
        proper = int(((mask != 0) & (mask != (1 << E) - 1)).sum())
        print("E", E, "cost", cases.CONDITIONED[k_cost][:2], "agent", a, "refused", int((first < H).sum()), "of 18,",
              "a proper subset refuses in", proper, "closest cost to the threshold", o["edge"][a].min())
        assert (first < H).any() and (first == H).any()
        assert proper >= 1
        assert o["edge"][a].min() > 1e-6
        assert np.array_equal(mask != 0, first < H)
        assert np.all(o["worst_max"][a] <= cases.ensemble_case(3, 9, E, cases.CONDITIONED[k_cost])["sim_thresh"][a])
    assert np.all(o["first_refused"][1] == H) and np.isnan(o["worst_max"][1]).all() and not o["refusing"][1].any()
