"""The CACLA matrix (tests/cacla_matrix_cases.py, tests/cacla_reference.py) without a GPU.

 * K.  R_oracle, the worst ratio of error to running bound (K = 1) of the three float64 NumPy oracles
   (tests/cacla_oracle.py, cacla_safe_oracle.py, cacla_ensemble_oracle.py, run for one step) over every one-step case,
   is measured here: R_oracle = 0.92 on this suite's CPU runs, so K = step_reference.k_from(R_oracle) = 4.  Never
   measured on a kernel.
 * COVERAGE.  The case list holds what it claims: every n, both signs of td, the relu pattern, every cost index with
   every ensemble size, every n_iter with one and with three agents, and the 28 instantiations, each launched by a
   test of part A or C of tests/test_cacla_matrix_gpu.py.
 * MARGINS.  Every decision of every one-step case lies more than K bounds from its edge (in fact more than 1e6 K),
   and the oracles' short runs keep the 1e-6 rule.  None is skipped: a case that failed this would fail here.
 * THE BOUND IS NOT VACUOUS.  Six mutants of the reference each leave it at every n in at least one case.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, observed

import oracle

import cacla_matrix_cases as mc
import cacla_reference as cr
import step_reference as sr

K = mc.K_MEASURED


def test_r_oracle_fixes_k():
    per_n = {n: mc.oracle_ratios(n) for n in mc.NS}
    r = max(per_n.values())
    observed("cacla_matrix_cpu", {"R_oracle": r, "R_oracle_per_n": {str(n): v for n, v in per_n.items()},
                                  "K": sr.k_from(r)})
    assert sr.k_from(r) == K == 4.0, (r, per_n)
    assert abs(r - mc.R_ORACLE_RECORDED) <= 0.05 * mc.R_ORACLE_RECORDED, r
    assert r <= 0.25 * K                                       # the oracles are inside every bound, by the factor 4


@pytest.mark.parametrize("n", mc.NS)
def test_the_inputs_are_legible(n):
    d = 2 * n + 2
    for regime in mc.REGIMES:
        c, ref = mc.one_step(n, regime), mc.reference(n, regime)
        assert len(np.unique(c["w"])) == c["w"].size == n * cr.net_doubles(n)
        assert (c["state"] != 0).all() and len(np.unique(c["state"])) == d
        assert (c["state"] != oracle.reset(oracle.OracleParams.make(n))).all()          # not the reset state
        assert np.abs(c["state"][2::2]).max() < np.pi and (c["noise"] != 0).all()
        codes = set()
        for net in range(n):
            on = ref["forward"]["on"][net]
            assert np.array_equal(on, mc.relu_code(n, net))
            assert (on[0::2] != on[1::2]).all() and on.sum() >= 3 and (~on).sum() >= 3
            codes.add(tuple(on))
        assert len(codes) == n
        assert (ref["td"].value > 0) == (regime == "up") and ref["actor_updates"] == int(regime == "up")
        assert abs(float(ref["td"].value) - mc.TD_TARGET[regime]) <= 1e-12
    rows = mc.members(n, 64)
    assert len(np.unique(rows, axis=0)) == 64 and (rows > 0).all() and np.array_equal(mc.members(n, 1)[0], mc.SIM)


def test_the_case_list_covers_what_it_claims():
    assert mc.NS == tuple(range(2, 9)) and mc.N_ITERS == (1, 2, 63, 64, 65, 129) and mc.MEMBERS == (1, 5, 64)
    assert {mc.run_agents(t) for t in mc.N_ITERS} == {1, 3}
    for n in mc.NS:
        assert mc.costs(n) == [(1, 0), (0, 0), (0, 1), (0, 3), (0, 2 * n), (0, 2 * n + 1)]
        cases = mc.gated_cases(n)
        for E in mc.MEMBERS:
            assert {ci for e, ci, _ in cases if e == E} == set(range(6)), (n, E)
        for ci in range(6):                                    # the single-simulator kernel: both verdicts at every cost
            assert {v for e, c, v in cases if e == 1 and c == ci} >= {"refuse"}
            assert {v for e, c, v in cases if e == 1 and c == ci} & {"admit", "violate"}
        verdicts = {v for _, _, v in cases}
        assert verdicts == set(mc.VERDICTS), (n, verdicts)
        for key in cases:
            ref, want = mc.gated_reference(n, *key), key[2]
            assert ref["admitted"] == (want in ("admit", "violate"))
            if ref["admitted"]:
                assert ref["violation"] == (want == "violate") and ref["member_in"].all()
            elif want == "split":
                assert 0 < ref["member_in"].sum() < key[0]
            else:
                assert not ref["member_in"].any()
    assert len(mc.INSTANTIATIONS) == len(set(mc.INSTANTIATIONS)) == 28
    reached = mc.reached_by()
    assert set().union(*map(set, reached.values())) == set(mc.INSTANTIATIONS)
    for kernel, n, train in mc.INSTANTIATIONS:                 # each by part A and by part C
        assert sum((kernel, n, train) in v for name, v in reached.items() if name.startswith("test_a_")) >= 1
        assert sum((kernel, n, train) in v for name, v in reached.items() if name.startswith("test_c_")) >= 1
    source = open(os.path.join(ROOT, "tests", "test_cacla_matrix_gpu.py")).read()
    for name in reached:
        assert re.search(rf"^def {name}\(", source, flags=re.M), name


@pytest.mark.parametrize("n", mc.NS)
def test_every_decision_is_far_from_its_edge(n):
    m = mc.margins(n)
    assert len(m) == 5 + len(mc.gated_cases(n))
    assert min(m.values()) > 1e6 * K, min(m.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("n", mc.NS)
def test_the_short_runs_keep_the_margin_rule(n):
    T = mc.N_ITERS[-1]                                         # the shorter runs are this one's prefixes
    some = dict(admitted=0, refused=0, violations=0, updates=0, idle=0)
    for agent in range(3):
        o = mc.run_oracle(n, T, True, agent)
        assert min(o["min_td"], o["min_z"]) >= 1e-6, (agent, o["min_td"])
        assert np.abs(o["weights"]).max() <= mc.RUN_WEIGHT_LIMIT             # 1e-9 absolute is for values of order one
        assert mc.run_oracle(n, T, False, agent)["min_z"] >= 1e-6
        some["updates"] += o["actor_updates"]
        some["idle"] += T - o["actor_updates"]
        for ens in (False, True):
            g = mc.run_gated_oracle(n, T, ens, agent)
            assert min(g["min_sim_margin"], g["min_real_margin"], g["min_td"]) >= 1e-6, (agent, ens)
            assert np.abs(g["weights"]).max() <= mc.RUN_WEIGHT_LIMIT
            some["admitted"] += g["counters"][0]
            some["refused"] += T - g["counters"][0]
            some["violations"] += g["counters"][1]
    assert some.pop("idle") >= 1 and min(some.values()) >= 4, some   # both branches of every decision are taken
    first = mc.run_gated_oracle(n, 1, False)                   # the run of one step is admitted: it has a reward
    assert first["counters"][0] == 1


MUTANTS = {1: "the gradient uses the updated W2", 2: "V(s') is taken after the critic's update",
           3: "the actors update when td < 0", 4: "b2 is not updated", 5: "the gradient's x is the new state",
           6: "the actor's step is alpha * action"}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
@pytest.mark.parametrize("n", mc.NS)
def test_a_mutant_of_the_reference_leaves_the_bound(n, mutant):
    shown = {}
    for regime in mc.REGIMES:
        ref = mc.reference(n, regime)
        wrong = mc.reference(n, regime, mutant=mutant)["weights"].value.astype(np.float64)
        shown[regime] = sr.ratio(wrong, ref["weights"])
        # and the right restatement in float64 is inside it
        assert sr.ratio(mc.oracle_step(n, regime)["weights"], ref["weights"]) <= 0.25 * K
    assert max(shown.values()) > K, (MUTANTS[mutant], shown)
    if mutant == 3:
        assert shown["down"] > K and shown["up"] <= 1.0     # td > 0: the same rule, only the rounding to double is left
