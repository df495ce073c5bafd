"""The rollout matrix (tests/rollout_matrix_cases.py) without a GPU: that its list of instantiations IS what the
library holds, that its loop-crossing cases cross the loops, and that its references are usable.

 * COVERAGE.  The kernel symbols of the built library whose names are rollout_row_kernel, rollout_oct3_kernel,
   rollout_octp3_kernel, rollout_octl3_kernel, rollout_quad3_kernel or rollout_kernel<N, ..> (the names alone: the
   safe-exploration kernels safe_rollout_* contain them and are other kernels), the twin model's included: each is
   named by exactly one entry of INSTANTIATIONS, and each entry exists.  A template argument added later fails here
   until it has a case; every entry is reached by a launch of the GPU test.
 * CROSSINGS.  On the oracle's trajectories the restated loop control shows, for each n = 4..8, a wave that goes
   unchecked -> checked, one that goes checked -> unchecked, and a wave in the checked loop while three of its rollouts
   are below 10 rad/s; both kinds of crossing happen at steps that are no multiple of four; no evaluated test comes
   closer than 1e-5 rad to its threshold of 0.04 rad (a kernel within 1e-9 of the oracle takes the oracle's loops).
 * REFERENCES.  Every oracle trajectory is finite, and inputs scaled by 1 + 1e-13 move the oracle's own trajectory
   by at most 1e-10: a tenth of the bound the GPU test holds the kernels to.  The twin cases too (first run: at
   most 4.7e-12 at any n).
"""
import os
import re
import shutil

import numpy as np
import pytest

from test_loop_placement import LIB, LLVM, _disassemble

import rollout_matrix_cases as mc

needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and shutil.which(f"{LLVM}/llvm-objdump")),
                                 reason="needs the built library and the ROCm llvm tools")
MARGIN = 1e-5                  # rad, of 4 h |thetadot| from kTripSlack


def _launched():
    """The entries of INSTANTIATIONS that the launches of the GPU test reach (quad: its child process)."""
    out = set()
    for form, n in mc.FORMS:
        for ars in (False, True):
            for _, traj, mom, flags in mc.variants(form):
                out.add(mc.instantiation_of(form, n, ars, traj, mom, flags))
                if form == "oct3":
                    out.add(mc.instantiation_of(form, n, ars, traj, mom, flags, quad_env=True))
    return out


def test_the_list_has_88_entries_and_the_gpu_test_launches_each():
    assert len(mc.INSTANTIATIONS) == 88 and len({i.symbol for i in mc.INSTANTIATIONS}) == 88
    assert _launched() == set(mc.INSTANTIATIONS)
    assert [sum(i.symbol.startswith(k) for i in mc.INSTANTIATIONS) for k in mc.KERNEL_NAMES] == [40, 8, 2, 2, 8, 28]
    assert sum(i.symbol.endswith("ELb1E") and i.form == "twin" for i in mc.INSTANTIATIONS) == 14
    # the twin model runs the lane form's shapes, all of them
    assert mc.plain_shapes("twin") == mc.plain_shapes("lane") and mc.ars_shapes("twin") == mc.ars_shapes("lane")
    assert [v[:3] for v in mc.variants("twin")] == [v[:3] for v in mc.variants("lane")]


@needs_tools
def test_every_compiled_instantiation_is_listed_once():
    names = [k[:k.index("ILi")] if k.endswith("ILi") else k for k in mc.KERNEL_NAMES]
    # <length><name>I: the Itanium spelling of a template's own name, so that safe_rollout_row_kernel is not taken
    pattern = re.compile("(?:" + "|".join(f"{len(k)}{k}I" for k in names) + ")")
    symbols = sorted({l.split("<", 1)[1][:-2] for l in _disassemble()
                      if l.startswith("0000") and l.endswith(">:") and pattern.search(l)})
    assert len(symbols) == 88, (len(symbols), symbols)
    for s in symbols:
        named_by = [i.symbol for i in mc.INSTANTIATIONS if i.symbol + "E" in s]
        assert len(named_by) == 1, (s, named_by)
    for i in mc.INSTANTIATIONS:
        assert sum(i.symbol + "E" in s for s in symbols) == 1, (i, "is not in the library")


def _transitions(loop, to):
    return [t for t in range(1, len(loop)) if loop[t] == to and loop[t - 1] != to]


@pytest.mark.parametrize("n", sorted(mc.CROSSING))
def test_the_crossing_cases_cross_the_loops(n):
    inp = mc.crossing_case(n)
    assert inp["H"] <= 48 and 12 <= inp["policies"].shape[0] <= 16
    ref = mc.reference(inp)
    assert np.isfinite(ref["traj"]).all()
    waves = mc.wave_loops(inp, ref)
    assert min(w[1] for w in waves) > MARGIN
    # wave 0: from rest, driven past 10 rad/s
    assert not ref["start"][:4, 3::2].any() and waves[0][0][0] == mc.UNCHECKED
    assert _transitions(waves[0][0], mc.CHECKED)
    # wave 1: starts in the checked loop, falls out of it and is taken back, neither at a multiple of four
    assert waves[1][0][0] == mc.CHECKED
    out, back = _transitions(waves[1][0], mc.UNCHECKED), _transitions(waves[1][0], mc.CHECKED)
    assert out and back and out[0] % 4 != 0 and any(t % 4 for t in back), (out, back)
    # wave 2: in the checked loop for one rollout's sake
    loop, _, speed = waves[2]
    assert ((loop == mc.CHECKED) & ((speed < 10.0).sum(axis=1) == 3)).any()
    # wave 3: partial, never leaves the unchecked trips: both loops run in one workgroup
    assert len(waves) == 4 and speed.shape[1] == 4 and waves[3][2].shape[1] == 2
    assert (waves[3][0] == mc.UNCHECKED).all()
    # as the ARS entry point runs it: every rollout from rest
    rest = mc.crossing_case(n, from_rest=True)
    assert np.array_equal(rest["policies"], inp["policies"])
    ref = mc.reference(rest)
    waves = mc.wave_loops(rest, ref)
    assert np.isfinite(ref["traj"]).all() and min(w[1] for w in waves) > MARGIN
    assert all(w[0][0] == mc.UNCHECKED for w in waves)
    assert _transitions(waves[0][0], mc.CHECKED) and _transitions(waves[1][0], mc.CHECKED)
    loop, _, speed = waves[2]
    mixed = (loop == mc.CHECKED) & ((speed < 10.0).sum(axis=1) >= 2) & ((speed > 10.0).sum(axis=1) >= 1)
    assert mixed.any()


def _launches(form, n):
    model = mc.model_of(form)
    for v2 in (False, True):
        for H, R, s0 in mc.plain_shapes(form):
            yield mc.plain_inputs(n, H, R, s0, v2, model)
        for H, n_dir, dir_begin in mc.ars_shapes(form):
            yield mc.ars_inputs(n, H, n_dir, dir_begin, v2, model)
    if n in mc.CROSSING and form == "row":
        yield mc.crossing_case(n)
        yield mc.crossing_case(n, from_rest=True)


@pytest.mark.parametrize("form,n", mc.FORMS)
def test_the_references_are_finite_and_stable(form, n):
    worst = 0.0
    for inp in _launches(form, n):
        a, b = mc.reference(inp), mc.reference(inp, scale=1.0 + 1e-13)
        assert np.isfinite(a["traj"]).all() and np.isfinite(a["returns"]).all()
        moved = max(np.abs(a["traj"] - b["traj"]).max(initial=0.0), np.abs(a["returns"] - b["returns"]).max())
        worst = max(worst, moved)
        assert moved <= mc.STABLE, (inp["n"], inp["H"], inp["policies"].shape, moved)
    print(f"{form} n = {n}: inputs scaled by 1 + 1e-13 move the oracle by at most {worst:.1e}")


def test_the_ars_inputs_would_show_a_wrong_slice():
    """The rows of deltas before and behind a launch's slice are a thousand times the slice's: read in place of a
    direction (dir_begin dropped, or the rollout's index taken for its direction's) they move every trajectory that
    depends on them far beyond the bound, and there are enough of them behind the slice for the second mistake to stay
    inside the array."""
    inp = mc.ars_inputs(5, 13, 7, 3, False)
    assert inp["deltas"].shape[0] == 3 + 2 * 7 + mc.EXTRA_ROWS
    assert np.abs(inp["deltas"][:3]).min() >= mc.POISON and np.abs(inp["deltas"][10:]).min() >= mc.POISON
    good = mc.reference(inp)["traj"]                 # (from rest and over 13 steps the returns themselves are ~ 1e-8)
    dropped = mc.ars_policies(inp["policy"], inp["deltas"], inp["nu"], 0, 7)          # dir_begin dropped
    bad = mc.reference(dict(inp, policies=dropped))["traj"]
    assert not (np.abs(bad - good).max(axis=(1, 2)) <= 1e3 * mc.TOL).any()
    sign = np.where(np.arange(14) % 2, -1.0, 1.0)[:, None, None]                      # rollout r reads row dir_begin + r
    by_rollout = inp["policy"] + sign * (inp["nu"] * inp["deltas"][3:17])
    bad = mc.reference(dict(inp, policies=by_rollout))["traj"]
    assert not (np.abs(bad - good).max(axis=(1, 2)) <= 1e3 * mc.TOL)[1:].any()
