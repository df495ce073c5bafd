"""The batch families (tests/batch_kernel_cases.py) without a GPU: that the list of instantiations IS what the library
holds, and that the GPU tests' parameter lists reach every entry of it.

 * COVERAGE.  The kernel symbols of the built library whose names begin with ars_gate_, ars_multi_ or ars_counted_
   (the names alone; that covers ars_gate_multi_ and ars_gate_ens_): each is named by exactly one entry of
   INSTANTIATIONS, and each entry exists.  A template argument added later fails here until it has a case.
 * REACH.  launches() derives, from the parameter lists that the GPU tests are parametrized with and a restatement of
   the dispatch, which kernel every case launches: every entry is launched by at least one test, and no case launches
   a kernel that is not an entry.
"""
import os
import re
import shutil

import pytest

from test_loop_placement import LIB, LLVM, _disassemble

import batch_kernel_cases as bc

needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and shutil.which(f"{LLVM}/llvm-objdump")),
                                 reason="needs the built library and the ROCm llvm tools")


def test_the_list_has_120_entries_and_a_gpu_test_launches_each():
    assert len(bc.INSTANTIATIONS) == 120 and len({i.symbol for i in bc.INSTANTIATIONS}) == 120
    per_family = {f: sum(i.family == f for i in bc.INSTANTIATIONS) for f in list(bc.FAMILY_NAMES) + ["fold"]}
    assert per_family == dict(gate=21, gate_multi=21, gate_ens=21, counted=28, multi=28, fold=1)
    reached = bc.launched_by()
    listed = {i.symbol for i in bc.INSTANTIATIONS}
    assert set(reached) <= listed, sorted(set(reached) - listed)          # a case launches a kernel that is no entry
    missing = [i for i in bc.INSTANTIATIONS if bc.test_of(i) is None]
    assert not missing, ("no GPU test launches", missing)
    for i in bc.INSTANTIATIONS:
        assert bc.test_of(i).startswith("tests/test_") and "::test_" in bc.test_of(i)


def test_the_dispatch_restatement_at_its_thresholds():
    """form_of against the rules of plan_rollouts: the caps are on the slots of the whole launch, FLAG_ROLLOUT_QUAD
    lifts them without choosing the quad form, SWIMMER_N3_KERNEL=quad does choose it, n = 2 has the lane form only."""
    assert [bc.form_of(3, "auto", s) for s in (2, 8192, 8194, 16384, 16386)] == ["oct3", "oct3", "quad3", "quad3", "lane"]
    assert [bc.form_of(3, "quad", s) for s in (2, 8194, 16386)] == ["oct3", "quad3", "quad3"]
    assert [bc.form_of(3, "auto", s, quad_env=True) for s in (2, 8194)] == ["quad3", "quad3"]
    assert [bc.form_of(6, "auto", s) for s in (2, 8192, 8194)] == ["row", "row", "lane"]
    assert bc.form_of(2, "auto", 2) == "lane" and bc.form_of(6, "lane", 2) == "lane" and bc.form_of(6, "twin", 2) == "lane"
    assert bc.batch_slots(3, 7) == 48 and bc.batch_slots(3, 8) == 48 and bc.batch_slots(3, 9) == 96


@needs_tools
def test_every_compiled_instantiation_is_listed_once():
    # _GLOBAL__N_1<length><name>: the Itanium spelling of a name in the anonymous namespace, the prefix at its start
    pattern = re.compile(r"_GLOBAL__N_1\d+(?:" + "|".join(bc.PREFIXES) + r")\w*?kernel[IE]")
    symbols = sorted({l.split("<", 1)[1][:-2] for l in _disassemble()
                      if l.startswith("0000") and l.endswith(">:") and pattern.search(l)})
    assert len(symbols) == 120, (len(symbols), symbols)
    for s in symbols:
        named_by = [i.symbol for i in bc.INSTANTIATIONS if "_GLOBAL__N_1" + i.symbol in s]
        assert len(named_by) == 1, (s, named_by)
    for i in bc.INSTANTIATIONS:
        assert sum("_GLOBAL__N_1" + i.symbol in s for s in symbols) == 1, (i, "is not in the library")
