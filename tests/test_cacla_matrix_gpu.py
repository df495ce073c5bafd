"""The CACLA swimmer kernels (cacla_kernel<N, TRAIN>, cacla_safe_kernel<N>, cacla_ensemble_kernel<N>, n = 2..8: all 28
instantiations) on the GPU against tests/cacla_reference.py on the cases of tests/cacla_matrix_cases.py.

 A. ONE STEP, per entry: reward, state, every weight entry, the look-ahead cost within K times the reference's running
    bound; actor_updates, counters, records, verdicts equal; what must not move keeps its bits.
 B. THE EDGES, made exact from the kernel's own outputs: td == 0 and one ulp either side, a NaN gamma, z == 0 against
    z = 2^-1000, both thresholds at equality, one ulp inside, and NaN.
 C. SHORT RUNS of 1, 2, 63, 64, 65 and 129 steps against the float64 oracles at the standing 1e-9, masks and counters
    equal (the oracle's own run keeps every decision 1e-6 from its edge: asserted first).
 D. GUARDS: every in/out and output array of every launch here lies between 64 guard entries on each side (NaN, -7),
    with one and three agents, the optional outputs given and NULL.

K = 4: step_reference.k_from(R_oracle) with R_oracle = 0.92 measured on the float64 oracles without a GPU
(tests/test_cacla_matrix_cpu.py), never on a kernel.  Each test asserts its cases' margins before it compares; none is
skipped.  The kernels' observed ratios per kernel and n go to profiles/cacla_matrix_observed.json."""
import numpy as np
import pytest
import torch

import swimmer_amd as sw
from conftest import observed
from swimmer_amd.cacla import safe_kernels

import cacla_matrix_cases as mc
import step_reference as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = mc.K_MEASURED
GUARD = mc.GUARD
POISON = -7.25e77                     # an output entry that was never written
F64, I32 = torch.float64, torch.int32
_seen = {}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def t64(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=DEV)


class Guarded:
    """Device arrays that each sit in the middle of a buffer of guard entries (NaN for doubles, -7 for ints)."""

    def __init__(self):
        self.bufs = {}

    def add(self, name, init, dtype=F64):
        init = np.ascontiguousarray(init)
        buf = torch.full((init.size + 2 * GUARD,), float("nan") if dtype == F64 else -7, dtype=dtype, device=DEV)
        view = buf[GUARD:GUARD + init.size].view(init.shape)
        view.copy_(torch.as_tensor(init).to(dtype))
        self.bufs[name] = (buf, view)
        return view

    def collect(self):
        """{name: host array}, after asserting that every guard entry kept its bits."""
        torch.cuda.synchronize()
        out = {}
        for name, (buf, view) in self.bufs.items():
            host = buf.cpu().numpy()
            edge = np.concatenate([host[:GUARD], host[GUARD + view.numel():]])
            assert len(edge) == 2 * GUARD
            if host.dtype == np.float64:
                assert same_bits(edge, np.full(2 * GUARD, np.nan)), (name, edge)
            else:
                assert (edge == -7).all(), (name, edge)
            out[name] = host[GUARD:GUARD + view.numel()].reshape(tuple(view.shape)).copy()
        return out


def agent_of(case, noise=None):
    return (case["w"], case["state"], case["noise"][None] if noise is None else noise, case["gamma"], case["alpha"])


def run_plain(n, train, agents, optional=True):
    """sw_cacla_run_f64 for agents [(w, state, noise [T, m], gamma, alpha)] -> dict of host arrays."""
    A, T = len(agents), agents[0][2].shape[0]
    g = Guarded()
    w = g.add("weights", np.stack([a[0] for a in agents]))
    s = g.add("state", np.stack([a[1] for a in agents]))
    r = g.add("rewards", np.full((A, T), POISON))
    upd = g.add("actor_updates", np.zeros(A), I32) if optional else None
    status = g.add("status", np.zeros(A), I32) if optional else None
    sw.kernels.cacla_run(sw.SwParams.make(n), T, train, t64([a[3] for a in agents]), t64([a[4] for a in agents]),
                         t64(np.stack([a[2] for a in agents])), w, s, rewards=r, actor_updates=upd, status=status)
    return g.collect()


def run_gated(n, agents, gates, ensemble, optional=True, t_begin=0, gated=None):
    """sw_cacla_safe_run_f64 or sw_cacla_safe_ensemble_run_f64; gates: one dict(sims [E, 3], kind, index, sim_thresh,
    real_thresh) per agent, kind, index and E common."""
    A, T = len(agents), agents[0][2].shape[0]
    E = len(gates[0]["sims"])
    g = Guarded()
    w = g.add("weights", np.stack([a[0] for a in agents]))
    s = g.add("state", np.stack([a[1] for a in agents]))
    last = g.add("last", np.full(A, np.nan))
    r = g.add("rewards", np.full((A, T), POISON))
    counters = g.add("counters", np.zeros((A, 3)), I32)
    first = g.add("first", np.full(A, -1), I32)
    rec = g.add("admitted", np.full((A, T), -3), I32) if optional else None
    status = g.add("status", np.zeros(A), I32) if optional else None
    args = (sw.SwParams.make(n), T, t_begin, t64([a[3] for a in agents]), t64([a[4] for a in agents]),
            t64(np.stack([a[2] for a in agents])),
            torch.as_tensor(np.asarray([1] * A if gated is None else gated, dtype=np.int32), device=DEV))
    thr = (t64([q["sim_thresh"] for q in gates]), t64([q["real_thresh"] for q in gates]), gates[0]["kind"],
           gates[0]["index"], w, s, last, counters, first)
    if ensemble:
        worst = g.add("worst", np.full((A, T), POISON)) if optional else None
        refusals = g.add("refusals", np.zeros((A, E)), I32) if optional else None
        safe_kernels.cacla_safe_ensemble_run(*args, t64(np.stack([q["sims"] for q in gates])), *thr, rewards=r,
                                             admitted_rec=rec, worst_rec=worst, member_refusals=refusals,
                                             status=status)
    else:
        assert E == 1
        safe_kernels.cacla_safe_run(*args, t64(np.stack([q["sims"][0] for q in gates])), *thr, rewards=r,
                                    admitted_rec=rec, status=status)
    return g.collect()


def note(kernel, n, figure):
    per = _seen.setdefault(kernel, {})
    per[str(n)] = max(per.get(str(n), 0.0), float(figure))
    observed("cacla_matrix_observed", {"K": K, "R_oracle": mc.R_ORACLE_RECORDED, "ratios": _seen})


def within(kernel, n, got, a, ref, gated=False):
    """Agent a of a one-step launch against a reference step: every ratio printed, kept, and <= K."""
    one = dict(rewards=got["rewards"][a], weights=got["weights"][a], state=got["state"][a],
               worst=got["worst"][a] if "worst" in got else None)
    fig = mc.ratios(one, ref, gated)
    print(kernel, n, a, fig)
    note(kernel, n, max(fig.values()))
    assert max(fig.values()) <= K, (kernel, n, a, fig)


SHAPES = ((1, False), (3, True))      # agents and whether the optional outputs are given: both, in every test of A


# ---- A: one step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mc.NS)
def test_a_one_step_training(n):
    for A, optional in SHAPES:
        regimes = [mc.REGIMES[a % 2] for a in range(A)]
        refs = [mc.reference(n, r) for r in regimes]
        assert all(ref["edge"] > K for ref in refs)
        got = run_plain(n, True, [agent_of(mc.one_step(n, r)) for r in regimes], optional)
        for a, (regime, ref) in enumerate(zip(regimes, refs)):
            within("cacla_kernel_train", n, got, a, ref)
            if regime == "down":                                # only the critic moved
                assert same_bits(got["weights"][a, :n - 1], mc.one_step(n, regime)["w"][:n - 1])
        if optional:
            assert got["actor_updates"].tolist() == [ref["actor_updates"] for ref in refs] == [1, 0, 1]
            assert not got["status"].any()


@pytest.mark.parametrize("n", mc.NS)
def test_a_one_step_without_training(n):
    for A, optional in SHAPES:
        regimes = [mc.REGIMES[a % 2] for a in range(A)]
        refs = [mc.reference(n, r, False) for r in regimes]
        assert all(ref["edge"] > K for ref in refs)
        got = run_plain(n, False, [agent_of(mc.one_step(n, r)) for r in regimes], optional)
        for a, (regime, ref) in enumerate(zip(regimes, refs)):
            within("cacla_kernel_eval", n, got, a, ref)
            assert same_bits(got["weights"][a], mc.one_step(n, regime)["w"])
        if optional:
            assert not got["actor_updates"].any() and not got["status"].any()


def check_gated_step(kernel, n, got, a, ref, case, t_begin, optional):
    """Agent a of a gated one-step launch: the step of `ref` when admitted, nothing at all when refused."""
    if ref["admitted"]:
        within(kernel, n, got, a, ref, gated=True)
        assert got["counters"][a].tolist() == [1, int(ref["violation"]), ref["actor_updates"]]
        assert same_bits(got["last"][a], got["rewards"][a, 0]) and got["first"][a] == -1
    else:
        assert same_bits(got["weights"][a], case["w"]) and same_bits(got["state"][a], case["state"])
        assert same_bits(got["rewards"][a], [np.nan]) and same_bits(got["last"][a], np.nan)
        assert got["counters"][a].tolist() == [0, 0, 0] and got["first"][a] == t_begin
        if "worst" in got:
            fig = sr.ratio(got["worst"][a, 0], ref["worst"])
            note(kernel, n, fig)
            assert fig <= K, fig
    if optional:
        assert got["admitted"][a].tolist() == [int(ref["admitted"])] and got["status"][a] == 0
        if "refusals" in got:
            assert np.array_equal(got["refusals"][a], (~ref["member_in"]).astype(np.int32))


def gated_step_launch(n, key, ensemble, A, optional, t_begin):
    """A one-step gated case in agents 0 and 2; agent 1 of three is ungated and in the `down` regime."""
    case, down = mc.one_step(n, "up"), mc.one_step(n, "down")
    ref, gate = mc.gated_reference(n, *key), mc.gate(n, *key)
    assert ref["edge"] > K and mc.reference(n, "down")["edge"] > K
    gated = [1, 0, 1][:A]
    got = run_gated(n, [agent_of(case if q else down) for q in gated], [gate] * A, ensemble, optional, t_begin, gated)
    kernel = "cacla_ensemble_kernel" if ensemble else "cacla_safe_kernel"
    for a, q in enumerate(gated):
        if q:
            check_gated_step(kernel, n, got, a, ref, case, t_begin, optional)
        else:
            within(kernel, n, got, a, mc.reference(n, "down"))
            assert got["counters"][a, 0] == 1 and got["counters"][a, 2] == 0 and got["first"][a] == -1
            assert same_bits(got["weights"][a, :n - 1], down["w"][:n - 1])
            if optional and ensemble:
                assert same_bits(got["worst"][a], [np.nan]) and not got["refusals"][a].any()


@pytest.mark.parametrize("n", mc.NS)
def test_a_one_step_gated(n):
    keys = [key for key in mc.gated_cases(n) if key[0] == 1]
    assert len(keys) == 12
    for i, key in enumerate(keys):
        gated_step_launch(n, key, False, *SHAPES[i % 2], t_begin=7 * i)


@pytest.mark.parametrize("n", mc.NS)
def test_a_one_step_ensemble(n):
    keys = mc.gated_cases(n)
    assert {key[0] for key in keys} == set(mc.MEMBERS)
    for i, key in enumerate(keys):
        # worst_rec and member_refusals are compared where they are given: every third launch goes without
        gated_step_launch(n, key, True, *SHAPES[int(i % 3 != 2)], t_begin=5 * i)


# ---- B: the edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mc.NS)
def test_b_td_equal_to_zero_moves_no_actor(n):
    case, m = mc.one_step(n, "up"), n - 1
    first = run_plain(n, True, [agent_of(case)])
    r = first["rewards"][0, 0]                              # does not depend on the critic
    assert np.isfinite(r) and first["actor_updates"][0] == 1

    def with_b2(b2, gamma=0.0):
        w = case["w"].copy()
        w[m, -13:-1] = 0.0                                  # the critic's W2: V(s) = V(s') = b2 exactly
        w[m, -1] = b2
        return w, run_plain(n, True, [(w, case["state"], case["noise"][None], gamma, case["alpha"])])
    w, got = with_b2(r)                                     # td = (r + 0 * r) - r = 0: not > 0
    assert same_bits(got["rewards"], first["rewards"]) and same_bits(got["state"], first["state"])
    assert got["actor_updates"][0] == 0 and same_bits(got["weights"][0], w)
    w, got = with_b2(np.nextafter(r, -np.inf))              # td = one ulp: the actors take the step they took before
    assert got["actor_updates"][0] == 1
    assert same_bits(got["weights"][0, :m], first["weights"][0, :m])
    assert not same_bits(got["weights"][0, :m], w[:m])
    w, got = with_b2(np.nextafter(r, np.inf))               # td = minus one ulp
    assert got["actor_updates"][0] == 0 and same_bits(got["weights"][0, :m], w[:m])
    w, got = with_b2(r, gamma=np.nan)                       # a NaN td: no actor update, and the critic says so
    assert got["actor_updates"][0] == 0 and same_bits(got["weights"][0, :m], w[:m])
    assert np.isnan(got["weights"][0, m, -1])


@pytest.mark.parametrize("n", mc.NS)
def test_b_z_equal_to_zero_is_off(n):
    d, j = 2 * n + 2, mc.ZERO_UNIT
    unit = np.r_[j * d:(j + 1) * d, 12 * d + j, 12 * d + 12 + j]   # the unit's W1 row, b1 and W2 in a network
    for tiny in (False, True):
        case, ref = mc.one_step(n, "up", j, tiny), mc.reference(n, "up", zero_unit=j, tiny=tiny)
        assert ref["edge"] > K and ref["actor_updates"] == 1
        got = run_plain(n, True, [agent_of(case)])
        within("cacla_kernel_train", n, got, 0, ref)
        assert got["actor_updates"][0] == 1
        moved = got["weights"][0] != case["w"]
        assert moved[:, -1].all()                            # every b2 moved: every network took its update
        if tiny:                                             # z = 2^-1000 > 0: on, the reference's update (above)
            assert moved[:, unit[:d + 1]].all()
        else:                                                # z == 0: off, bit for bit
            assert same_bits(got["weights"][0][:, unit], case["w"][:, unit])


def host_cost(state, kind, index):
    return abs(state[index]) if kind == mc.COST_ABS_OBS else np.abs(state[3::2]).max()   # exact


@pytest.mark.parametrize("n", mc.NS)
def test_b_thresholds_at_equality(n):
    case = mc.one_step(n, "up")
    for ci in (0, 1 + n % 5):
        kind, index = mc.costs(n)[ci]
        gate = dict(sims=mc.members(n, 1), kind=kind, index=index, sim_thresh=np.inf, real_thresh=np.inf)
        seen = run_gated(n, [agent_of(case)], [gate], True)
        c, c_real = seen["worst"][0, 0], host_cost(seen["state"][0], kind, index)
        assert 0 < c < np.inf and 0 < c_real < np.inf and seen["counters"][0].tolist() == [1, 0, 1]
        for ensemble in (True, False):
            sim = [dict(gate, sim_thresh=t) for t in (c, np.nextafter(c, 0.0), np.nan)]
            got = run_gated(n, [agent_of(case)] * 3, sim, ensemble, t_begin=11)
            assert got["admitted"][:, 0].tolist() == [1, 0, 0], (ci, ensemble)      # cost <= sim_thresh: equality admits
            assert got["counters"].tolist() == [[1, 0, 1], [0, 0, 0], [0, 0, 0]]
            assert got["first"].tolist() == [-1, 11, 11] and not got["status"].any()
            assert np.isnan(got["rewards"][1:]).all() and same_bits(got["state"][0], seen["state"][0])
            for a in (1, 2):
                assert same_bits(got["weights"][a], case["w"]) and same_bits(got["state"][a], case["state"])
            if ensemble:
                assert same_bits(got["worst"][:, 0], [c] * 3) and got["refusals"][:, 0].tolist() == [0, 1, 1]
            real = [dict(gate, real_thresh=t) for t in (c_real, np.nextafter(c_real, 0.0), np.nan)]
            got = run_gated(n, [agent_of(case)] * 3, real, ensemble)
            assert got["counters"].tolist() == [[1, 0, 1], [1, 1, 1], [1, 0, 1]], (ci, ensemble)   # cost > real_thresh
            for a in range(3):                               # the thresholds change nothing else
                assert same_bits(got["weights"][a], seen["weights"][0]) and same_bits(got["state"][a], seen["state"][0])


# ---- C: short runs --------------------------------------------------------------------------------------------------------
def optional_at(n_iter):
    return n_iter not in (63, 65)                            # one launch with one agent and one with three go without


@pytest.mark.parametrize("train", (False, True))
@pytest.mark.parametrize("n", mc.NS)
def test_c_short_runs(n, train):
    worst = 0.0
    for T in mc.N_ITERS:
        A = mc.run_agents(T)
        want = [mc.run_oracle(n, T, train, a) for a in range(A)]
        assert all(min(o["min_td"], o["min_z"]) >= 1e-6 for o in want)
        ins = [mc.run_inputs(n, T, a) for a in range(A)]
        got = run_plain(n, train, ins, optional_at(T))
        for a, o in enumerate(want):
            fig = max(np.abs(got["rewards"][a] - o["rewards"]).max(), np.abs(got["weights"][a] - o["weights"]).max(),
                      np.abs(got["state"][a] - o["state"]).max())
            worst = max(worst, fig)
            assert fig <= 1e-9, (T, a, fig)
            if not train:
                assert same_bits(got["weights"][a], ins[a][0])
        if optional_at(T):
            assert got["actor_updates"].tolist() == [o["actor_updates"] for o in want] and not got["status"].any()
    print("short runs", n, train, worst)


@pytest.mark.parametrize("ensemble", (False, True))
@pytest.mark.parametrize("n", mc.NS)
def test_c_short_gated_runs(n, ensemble):
    worst = 0.0
    sims = mc.members(n, mc.RUN_MEMBERS) if ensemble else np.array([mc.SIM])
    for T in mc.N_ITERS:
        A = mc.run_agents(T)
        want = [mc.run_gated_oracle(n, T, ensemble, a) for a in range(A)]
        assert all(min(o["min_sim_margin"], o["min_real_margin"], o["min_td"]) >= 1e-6 for o in want)
        gates = [dict(sims=sims, kind=mc.RUN_COST[0], index=mc.RUN_COST[1], sim_thresh=mc.run_thresholds(n, a)[0],
                      real_thresh=mc.run_thresholds(n, a)[1]) for a in range(A)]
        got = run_gated(n, [mc.run_inputs(n, T, a) for a in range(A)], gates, ensemble, optional_at(T), t_begin=3)
        for a, o in enumerate(want):
            nan = np.isnan(o["rewards"])
            assert np.array_equal(np.isnan(got["rewards"][a]), nan)
            fig = max(np.abs(got["rewards"][a][~nan] - o["rewards"][~nan]).max(initial=0.0),
                      np.abs(got["weights"][a] - o["weights"]).max(), np.abs(got["state"][a] - o["state"]).max())
            assert tuple(got["counters"][a]) == tuple(o["counters"]), (T, a)
            assert got["first"][a] == (-1 if o["first_refused"] is None else 3 + o["first_refused"])
            assert same_bits(got["last"][a], got["rewards"][a, -1])
            if optional_at(T):
                assert np.array_equal(got["admitted"][a].astype(bool), o["admitted"]) and got["status"][a] == 0
                if ensemble:
                    fig = max(fig, np.abs(got["worst"][a] - o["worst"]).max())
                    assert np.array_equal(got["refusals"][a], o["member_refusals"])
            worst = max(worst, fig)
            assert fig <= 1e-9, (T, a, fig)
    print("short gated runs", n, ensemble, worst)


# ---- D: the weights of a neighbour ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2, 5))                        # 40 and 4 lanes behind the last network
def test_d_exactly_an_agents_own_weights_change(n):
    T = 65
    ins = [mc.run_inputs(n, T, a) for a in range(3)]
    ins[1] = ins[1][:4] + (0.0,)                             # alpha = 0: every step of this agent's update is + 0
    got = run_plain(n, True, ins)
    assert same_bits(got["weights"][1], ins[1][0]) and got["actor_updates"][1] > 0
    for a in (0, 2):                                         # and its neighbours are what they are alone
        alone = run_plain(n, True, [ins[a]])
        assert same_bits(got["weights"][a], alone["weights"][0]) and same_bits(got["rewards"][a], alone["rewards"][0])
        assert (got["weights"][a] != ins[a][0]).any(axis=1).all()                   # each of its own networks moved
