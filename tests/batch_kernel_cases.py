"""Every compiled instantiation of the batch families -- the kernels whose names begin with ars_gate_, ars_multi_,
ars_gate_multi_, ars_counted_ and ars_gate_ens_ -- with the GPU test that launches it.  These kernels are compared bit
for bit with single-agent launches (the roots: tests/test_rollout_matrix_gpu.py), so what can go unnoticed here is an
instantiation that no test launches: each row body is instantiated per N with register pressure and a loop pad of its
own, each lane body per N and per model.  No GPU here: tests/test_batch_kernels_cpu.py checks that INSTANTIATIONS is
what the built library holds and that the GPU tests' parameters reach every entry.

THE PARAMETER LISTS of those GPU tests live here, so that what is launched is derived from what is run and cannot be
kept by hand beside it:
  GATE_SHAPES          tests/test_safe_ars_agent_gpu.py  test_gate_kernel_against_ars_rollouts
  SAFE_BATCH_FORMS     tests/test_safe_batch_gpu.py      test_kernels_equal_their_single_agent_twins
  ENSEMBLE_FORMS       tests/test_ensemble_gate_gpu.py   test_members_equal_the_single_gate_and_the_fold_its_restatement
  MULTI_*, MORE_INSTANTIATIONS   tests/test_ars_multi_gpu.py   test_multi_rollouts_equal_single_agent_launches,
                                                               test_multi_rollouts_at_every_compiled_n_and_model
and QUAD_CHILDREN names the three tests that run the n = 3 cases once more with SWIMMER_N3_KERNEL=quad in a child.

form_of() restates the dispatch (plan_rollouts / plan_multi, csrc/swimmer_abi.hip): the form names "lane" and "twin"
force one rollout per lane, "twin" with the twin model; otherwise n = 3 takes the mirror-quad form up to 8192 rollout
slots and the quad form beyond (or everywhere with SWIMMER_N3_KERNEL=quad), n = 4..8 the row form up to 8192 slots,
and everything else the lane form.  A batch launch counts slots over the whole launch: agents (times members) times
2N rounded up to 16.

Symbols are spelt <length><name>[I<template arguments>E]E, the Itanium spelling of a name inside its namespace: the
length in front keeps ars_gate_kernel from being found in ars_gate_row_kernel.
"""
import collections

from swimmer_amd import _lib

MOM_GROUP = 16                # rollout slots per moment row: the granule of a batch launch (kMomGroup)
OCT_MAX = 8192                # kOctMaxRollouts
QUAD_MAX = 16384              # kQuadMaxRollouts
ROW_MAX = 8192                # kRowMaxRollouts

# ------------------------------------------------------------------------------------------------ the GPU tests' parameters
# test_gate_kernel_against_ars_rollouts: (n, N, form); V2 where N is odd
GATE_SHAPES = [(n, N, form) for n in range(2, 9) for N in (1, 7, 64, 2049) for form in ("auto", "lane")] + \
              [(3, N, "quad") for N in (1, 7, 64, 2049)] + [(3, 4097, "auto"), (6, 4097, "auto")] + \
              [(n, N, "twin") for n in range(2, 9) for N in (1, 7, 64)]

# test_kernels_equal_their_single_agent_twins: (n, form, id), S = 3 agents, N = 9, V1 and V2
SAFE_BATCH_FORMS = [(3, "auto", "mirror-quad"), (6, "auto", "row"), (2, "auto", "lane-n2"), (3, "lane", "lane-n3")] + \
                   [(n, "auto", f"row-n{n}") for n in (4, 5, 7, 8)] + \
                   [(n, "lane", f"lane-n{n}") for n in range(4, 9)] + \
                   [(n, "twin", f"twin-n{n}") for n in range(2, 9)]
SAFE_BATCH_S, SAFE_BATCH_N = 3, 9

# test_members_equal_the_single_gate_and_the_fold_its_restatement: (n, form, N), S = 3 agents of E = 3 members
ENSEMBLE_FORMS = [(3, "auto", 9), (4, "auto", 9), (5, "auto", 9), (6, "auto", 9), (7, "auto", 9), (8, "auto", 9),
                  (2, "auto", 9), (3, "lane", 9), (5, "lane", 9), (3, "twin", 9), (2, "auto", 33), (3, "lane", 33),
                  (5, "lane", 33), (3, "twin", 33)] + \
                 [(n, "lane", 9) for n in (4, 6, 7, 8)] + [(n, "twin", 9) for n in (2, 4, 5, 6, 7, 8)] + \
                 [(6, "twin", 33)]
ENSEMBLE_S, ENSEMBLE_E = 3, 3

# test_multi_rollouts_equal_single_agent_launches: the product of these, always with moments
MULTI_NS = [2, 3, 6]          # lane only, mirror-quad, row
MULTI_DIRS = [1, 7, 8, 9]     # 2N = 2, 14, 16, 18: below, just below, exactly, across a moment row
MULTI_AGENTS = [1, 3, 9]
MULTI_FORMS = ["auto", "lane"]

# test_multi_rollouts_at_every_compiled_n_and_model: (form, twin model, n, N, V2, moments asked for), S = 3 agents
MORE_INSTANTIATIONS = [
    ("auto", False, 4, 7, False, False), ("auto", False, 4, 7, True, True),
    ("auto", False, 4, 9, False, False), ("auto", False, 4, 9, True, True),
    ("auto", False, 5, 7, False, False), ("auto", False, 5, 7, True, True),
    ("auto", False, 5, 9, False, False), ("auto", False, 5, 9, True, True), ("auto", False, 5, 9, True, False),
    ("auto", False, 6, 7, False, False), ("auto", False, 6, 9, False, False),
    ("auto", False, 7, 7, False, False), ("auto", False, 7, 7, True, True),
    ("auto", False, 7, 9, False, False), ("auto", False, 7, 9, True, True),
    ("auto", False, 8, 7, False, False), ("auto", False, 8, 7, True, True),
    ("auto", False, 8, 9, False, False), ("auto", False, 8, 9, True, True),
    ("lane", False, 4, 9, False, True), ("lane", False, 4, 9, True, True),
    ("lane", False, 5, 9, False, True), ("lane", False, 5, 9, True, True),
    ("lane", False, 7, 9, False, True), ("lane", False, 7, 9, True, True),
    ("lane", False, 8, 9, False, True), ("lane", False, 8, 9, True, True),
    ("lane", True, 2, 9, False, True), ("lane", True, 2, 9, True, True),
    ("lane", True, 3, 9, False, True), ("lane", True, 3, 9, True, True),
    ("lane", True, 4, 9, False, True), ("lane", True, 4, 9, True, True),
    ("lane", True, 5, 9, False, True), ("lane", True, 5, 9, True, True),
    ("lane", True, 6, 9, False, True), ("lane", True, 6, 9, True, True),
    ("lane", True, 7, 9, False, True), ("lane", True, 7, 9, True, True),
    ("lane", True, 8, 9, False, True), ("lane", True, 8, 9, True, True),
]
MORE_S = 3

QUAD_CHILDREN = {        # family -> the test whose child process runs n = 3, N = 9, S = 3 on the quad form
    "safe_batch": "tests/test_safe_batch_gpu.py::test_kernels_in_the_quad_form_in_a_child_process",
    "ensemble": "tests/test_ensemble_gate_gpu.py::test_the_quad_form_in_a_child_process",
    "multi": "tests/test_ars_multi_gpu.py::test_quad3_multi_form_in_a_child_process",
}


def flags_of(form):
    """sw_params.flags of a form name of these tests: kernel_flags' names and "twin"."""
    return _lib.FLAG_MODEL_TWIN | _lib.FLAG_ROLLOUT_LANE if form == "twin" else _lib.kernel_flags(form)


def more_id(form, twin, n, N, v2, with_moments):
    return f"{form}-{'twin' if twin else 'swimmer'}-n{n}-N{N}-{'V2' if v2 else 'V1'}-{'mom' if with_moments else 'nomom'}"


# ------------------------------------------------------------------------------------------------ instantiations
Inst = collections.namedtuple("Inst", "symbol family form n twin mom")
# family: gate | gate_multi | gate_ens | counted | multi | fold; form: oct3 | quad3 | row | lane; twin / mom: None where
# the kernel has no such template argument
FAMILY_NAMES = {"gate": "ars_gate", "gate_multi": "ars_gate_multi", "gate_ens": "ars_gate_ens",
                "counted": "ars_counted", "multi": "ars_multi"}
PREFIXES = ("ars_gate_", "ars_multi_", "ars_counted_")      # every family's name begins with one of these


def symbol_of(family, form, n, twin=False, mom=False):
    """The spelling of the kernel that a launch of `family` in `form` reaches."""
    b = lambda x: int(bool(x))
    if family == "fold":
        name, args = "ars_gate_fold_kernel", ""
    else:
        stem = FAMILY_NAMES[family]
        with_mom = family in ("counted", "multi")
        if form in ("oct3", "quad3"):
            name, args = f"{stem}_{form}_kernel", f"Lb{b(mom)}E" if with_mom else ""
        elif form == "row":
            name, args = f"{stem}_row_kernel", f"Li{n}E" + (f"Lb{b(mom)}E" if with_mom else "")
        else:
            name = "ars_gate_kernel" if family == "gate" else f"{stem}_lane_kernel"
            args = f"Li{n}ELb{b(twin)}E"
    return f"{len(name)}{name}" + (f"I{args}E" if args else "") + "E"


def _instantiations():
    out = [Inst(symbol_of("fold", None, None), "fold", None, None, None, None)]
    for family in FAMILY_NAMES:
        moms = (False, True) if family in ("counted", "multi") else (None,)
        for mom in moms:
            for form in ("oct3", "quad3"):
                out.append(Inst(symbol_of(family, form, 3, mom=mom), family, form, 3, None, mom))
            for n in range(4, 9):
                out.append(Inst(symbol_of(family, "row", n, mom=mom), family, "row", n, None, mom))
        for n in range(2, 9):
            for twin in (False, True):
                out.append(Inst(symbol_of(family, "lane", n, twin=twin), family, "lane", n, twin, None))
    return tuple(out)


INSTANTIATIONS = _instantiations()


# ------------------------------------------------------------------------------------------------ what the tests launch
def form_of(n, form, slots, quad_env=False):
    """plan_rollouts restated: the kernel form of a launch of `slots` rollout slots under the form name `form`."""
    if form in ("lane", "twin"):
        return "lane"
    uncapped = form == "quad"                          # FLAG_ROLLOUT_QUAD lifts the caps, it does not choose the quad form
    if n == 3 and (uncapped or slots <= QUAD_MAX):
        return "oct3" if not quad_env and slots <= OCT_MAX else "quad3"
    if 4 <= n <= 8 and (uncapped or slots <= ROW_MAX):
        return "row"
    return "lane"


def batch_slots(members, N):
    return members * ((2 * N + MOM_GROUP - 1) // MOM_GROUP) * MOM_GROUP


def _reach(out, test, family, n, form, slots, mom=False, quad_env=False):
    out.append((symbol_of(family, form_of(n, form, slots, quad_env), n, form == "twin", mom), test))


def _safe_batch(out, test, n, form, quad_env=False):
    """_check_form of tests/test_safe_batch_gpu.py: the single gate, the multi gate, the counted rollouts V1 and V2."""
    S, N = SAFE_BATCH_S, SAFE_BATCH_N
    _reach(out, test, "gate", n, form, 2 * N, quad_env=quad_env)
    _reach(out, test, "gate_multi", n, form, batch_slots(S, N), quad_env=quad_env)
    for v2 in (False, True):                         # moments are passed with V2 only
        _reach(out, test, "counted", n, form, batch_slots(S, N), mom=v2, quad_env=quad_env)


def _ensemble(out, test, n, form, N, quad_env=False):
    """_check_form of tests/test_ensemble_gate_gpu.py: the single gates, the member launch with E = 3 and E = 1, the
    fold, the multi gate."""
    S, E = ENSEMBLE_S, ENSEMBLE_E
    _reach(out, test, "gate", n, form, 2 * N, quad_env=quad_env)
    _reach(out, test, "gate_ens", n, form, batch_slots(S * E, N), quad_env=quad_env)
    _reach(out, test, "gate_ens", n, form, batch_slots(S, N), quad_env=quad_env)
    _reach(out, test, "gate_multi", n, form, batch_slots(S, N), quad_env=quad_env)
    out.append((symbol_of("fold", None, None), test))


def launches():
    """[(symbol, test id)]: every batch-family kernel that the GPU tests' parameters reach, with the test that does."""
    out = []
    for n, N, form in GATE_SHAPES:
        _reach(out, f"tests/test_safe_ars_agent_gpu.py::test_gate_kernel_against_ars_rollouts[{n}-{N}-{form}]", "gate",
               n, form, 2 * N)
    for n, form, name in SAFE_BATCH_FORMS:
        _safe_batch(out, f"tests/test_safe_batch_gpu.py::test_kernels_equal_their_single_agent_twins[{name}]", n, form)
    _safe_batch(out, QUAD_CHILDREN["safe_batch"], 3, "auto", quad_env=True)
    for n, form, N in ENSEMBLE_FORMS:
        _ensemble(out, "tests/test_ensemble_gate_gpu.py::test_members_equal_the_single_gate_and_the_fold_its_"
                       f"restatement[n{n}-{form}-N{N}]", n, form, N)
    _ensemble(out, QUAD_CHILDREN["ensemble"], 3, "auto", 9, quad_env=True)
    for n in MULTI_NS:
        for N in MULTI_DIRS:
            for S in MULTI_AGENTS:
                for form in MULTI_FORMS:
                    for v2 in ("V1", "V2"):
                        _reach(out, "tests/test_ars_multi_gpu.py::test_multi_rollouts_equal_single_agent_launches"
                                    f"[{n}-{N}-{S}-{form}-{v2}]", "multi", n, form, batch_slots(S, N), mom=True)
    for form, twin, n, N, v2, with_moments in MORE_INSTANTIATIONS:
        _reach(out, "tests/test_ars_multi_gpu.py::test_multi_rollouts_at_every_compiled_n_and_model"
                    f"[{more_id(form, twin, n, N, v2, with_moments)}]", "multi", n, "twin" if twin else form,
               batch_slots(MORE_S, N), mom=with_moments)
    # V1 agents without moments, as ARSAgentBatch launches them; the quad child runs V1 and V2 with moments and V1 without
    _reach(out, "tests/test_ars_multi_gpu.py::test_multi_rollouts_without_moments_and_status", "multi", 3, "auto",
           batch_slots(3, 9), mom=False)
    for mom in (True, False):
        _reach(out, QUAD_CHILDREN["multi"], "multi", 3, "auto", batch_slots(3, 9), mom=mom, quad_env=True)
    return out


def launched_by():
    """symbol -> the test ids that launch it, in the order of launches()."""
    out = collections.OrderedDict()
    for symbol, test in launches():
        if test not in out.setdefault(symbol, []):
            out[symbol].append(test)
    return out


def test_of(inst):
    """The first test that launches an entry (None: no test does -- tests/test_batch_kernels_cpu.py fails then)."""
    return launched_by().get(inst.symbol, [None])[0]
