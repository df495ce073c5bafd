"""Every compiled instantiation of the LQR kernel (lqr_cacla_kernel<NS, NA, MODE>: 8 shapes x plain / step threshold /
fixed threshold) and every cost code against tests/lqr_oracle.py, one launch of 67 agents x 100 steps per case
(tests/lqr_matrix_cases.py; tests/test_lqr_matrix_cpu.py checks that the cases exercise what is compared here).

Every agent and every step is compared.  Exact: the admitted record with its three flag values, the three counters,
status 0.  Within 1e-9 absolute -- the project's standing bound for runs of <= 1000 steps (tests/test_lqr_gpu.py) --
the state, action and reward records and the final F, V and state; the rows of steps with nothing admitted yet are not
meaningful (tests/lqr_oracle.py) and are the only ones left out.  Bit for bit: the three costs at ns = 1, split runs
and runs without records at the shapes with the longest unrolled loops.
"""
import functools

import numpy as np
import pytest

from conftest import observed
from swimmer_amd import kernels
from swimmer_amd.cacla import lqr

import lqr_matrix_cases as mc

pytestmark = pytest.mark.gpu

BOUND = 1e-9
CASES = tuple((ns, na, mode, cost) for ns, na in mc.SHAPES for mode, cost in mc.VARIANTS)
_seen = {}


def _launch(ns, na, mode, cost, parts=(mc.STEPS,), record=lqr.RECORDS):
    """The case on the kernel in launches of `parts` steps: ({record: [A, T, ..]}, Run.finals())."""
    c = mc.case(ns, na, mode, cost)
    run = lqr.Run(c["kind"], ns, na, cost, c["columns"], c["F0"], c["V0"], c["x0"])
    at = [0]

    def draw(n):
        at[0] += n
        return c["noise"][:, at[0] - n:at[0]]
    recs = [run.run(n, n, draw, record) for n in parts]
    assert at[0] == mc.STEPS
    return {k: np.concatenate([r[k] for r in recs], axis=1) for k in recs[0]}, run.finals()


@functools.lru_cache(maxsize=None)
def _whole(ns, na, mode, cost):
    return _launch(ns, na, mode, cost)


def _same(a, b, what):
    (rec_a, fin_a), (rec_b, fin_b) = a, b
    assert list(rec_a) == list(rec_b)
    for k in rec_a:
        assert np.array_equal(rec_a[k], rec_b[k]), (what, k)
    for name, x, y in zip(("F", "V", "state", "admitted", "violations", "actor_updates", "status"), fin_a, fin_b):
        assert np.array_equal(x, y), (what, name)


@pytest.mark.parametrize("ns,na,mode,cost", CASES)
def test_every_instantiation_against_the_oracle(ns, na, mode, cost):
    want = mc.oracle(ns, na, mode, cost)
    rec, (F, V, state, admitted, violations, actor_updates, status) = _whole(ns, na, mode, cost)
    assert rec["states"].shape == (mc.AGENTS, mc.STEPS, ns) and rec["actions"].shape == (mc.AGENTS, mc.STEPS, na)
    assert rec["rewards"].shape == rec["admitted"].shape == (mc.AGENTS, mc.STEPS)
    flags = np.stack([w["admitted_flags"] for w in want])
    meant = flags != kernels.LQR_NOTHING_YET                  # [A, T]: the rows that mean something
    fig = {}
    for name in ("states", "actions", "rewards"):
        diff = np.abs(rec[name] - np.stack([w[name] for w in want]))
        fig[name] = float(diff[meant].max())
    for name, got in (("F", F), ("V", V), ("state", state)):
        fig[name] = float(np.abs(got - np.stack([w[name] for w in want])).max())
    fig["flags_differing"] = int((rec["admitted"] != flags).sum())
    _seen[f"ns{ns}_na{na}_mode{mode}_cost{cost}"] = fig
    observed("lqr_matrix", _seen)
    assert np.array_equal(rec["admitted"], flags)             # every step, all three values
    for name, got in (("admitted", admitted), ("violations", violations), ("actor_updates", actor_updates)):
        assert np.array_equal(got, [w[name] for w in want]), name
    assert not status.any()
    for name in ("states", "actions", "rewards", "F", "V", "state"):      # one by one: a NaN figure fails
        assert fig[name] <= BOUND, (name, fig)


@pytest.mark.parametrize("mode", (mc.STEP, mc.FIXED))
@pytest.mark.parametrize("na", (1, 2))
def test_the_three_costs_are_one_function_of_one_coordinate(na, mode):
    """ns = 1: the same agents under the inf-, 2- and 1-norm; every output agrees bit for bit."""
    first = _whole(1, na, mode, mc.COSTS[0])
    assert first[1][3].min() < mc.STEPS                       # the gate did refuse: the cost was evaluated
    for cost in mc.COSTS[1:]:
        assert np.array_equal(mc.case(1, na, mode, cost)["columns"], mc.case(1, na, mode, mc.COSTS[0])["columns"])
        _same(first, _whole(1, na, mode, cost), cost)


@pytest.mark.parametrize("mode", (mc.STEP, mc.FIXED))
def test_splitting_the_largest_shape_changes_nothing(mode):
    """(4, 2), the 2-norm: 100 steps in one launch, as 37 + 63 and as 64 + 36 -- every input and output of a launch
    that the next one continues from (F, V, state, the last admitted record, the counters), at the longest loops."""
    tag = (4, 2, mode, kernels.LQR_COST_2)
    whole = _whole(*tag)
    for parts in ((37, 63), (64, 36)):
        _same(whole, _launch(*tag, parts=parts), parts)


@pytest.mark.parametrize("ns,na,mode", ((4, 2, mc.STEP), (3, 1, mc.FIXED)))
def test_without_records_the_finals_are_the_same(ns, na, mode):
    """All four record pointers NULL against all four records: F, V, state, counters and status identical."""
    tag = (ns, na, mode, kernels.LQR_COST_1)
    rec, fin = _launch(*tag, record=())
    assert rec == {}
    _same(({}, _whole(*tag)[1]), ({}, fin), "no records")
