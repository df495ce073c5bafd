"""The built machine code of rollout_octs3_kernel -- the lean mode of the packed record form with the NEIGHBOUR'S MATRIX
ENTRY (csrc/swimmer_rollout_octp3.inc with SW_OCTP_NEXT_E 1) -- read out of the library's gfx950 code objects (no GPU
needed), against rollout_octl3_kernel IN THE SAME LIBRARY, and the flag that keeps a launch on that kernel.

What the variant is for: a lane takes Q(i+1, i+2) from lane i+1 through two v_mov_b32_dpp instead of forming it with
v_mul_f64 + v_fma_f64 + v_mul_f64.  Per step of the hot loop, therefore (relative counts, which another compiler build
does not break; the counts are normalised per step, so they hold for a trip of any length):
* at least 3 fewer f64 instructions, at most 2 more DPP moves, at least 1 instruction fewer in all;
* still exactly one buffer store, no load, no scratch (in the loop or anywhere in the kernel);
* the range test still branches on vcc (one s_cbranch_vccnz per step).
Where the hot loop sits in its 64-byte line is a perf lint for one compiler build (see test_loop_placement.py)."""
import ctypes
import os
import re
import shutil

import pytest

from test_isa_contracts import _kernels
from test_loop_placement import LIB, LLVM, PINNED_COMPILER, ROOT, _backward_loops, _compiler, _disassemble
from test_packed_capture_isa import _hot_loop

needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and shutil.which(f"{LLVM}/llvm-objdump")),
                                 reason="needs the built library and the ROCm llvm tools")

# (the new kernel, the lean kernel it is measured against): ARS form, plain form
PAIRS = [("rollout_octs3_kernelILb1E", "rollout_octl3_kernelILb1E"),
         ("rollout_octs3_kernelILb0E", "rollout_octl3_kernelILb0E")]
LEAN_STEPS_PER_TRIP = 8
# (bytes of the hot loop's body, offset of its head inside a 64-byte line): the choice of the sweep over the eight
# even pads, profiles/r13_b_octs_pad_sweep.log
EXPECTED = {"rollout_octs3_kernelILb1E": (11288, 0), "rollout_octs3_kernelILb0E": (11288, 0)}   # pad 2, 16 steps


def test_flag_and_name():
    import swimmer_amd as sw
    assert sw._lib.FLAG_CAPTURE_LEAN_V1 == 128 and sw._lib.kernel_flags("lean_v1") == 128
    assert sw._lib.kernel_flags("packed_v1") == 16 and sw._lib.kernel_flags("split") == 8
    assert sw._lib.kernel_flags("auto") == 0
    flags = (sw._lib.FLAG_ROLLOUT_LANE, sw._lib.FLAG_ROLLOUT_QUAD, sw._lib.FLAG_MODEL_TWIN, sw._lib.FLAG_CAPTURE_SPLIT,
             sw._lib.FLAG_CAPTURE_PACKED_V1, sw._lib.FLAG_CAPTURE_LEAN_V1)
    assert len(set(flags)) == 6 and all(f & (f - 1) == 0 for f in flags)
    header = open(os.path.join(ROOT, "include", "swimmer_hip.h")).read()
    assert re.search(r"#define\s+SW_FLAG_CAPTURE_LEAN_V1\s+128\b", header)
    assert re.search(r"#define\s+SW_ABI_VERSION\s+3\b", header) and sw._lib.ABI_VERSION == 3
    with pytest.raises(sw.SwimmerHipError):
        sw._lib.kernel_flags("lean")


def test_at_most_one_capture_flag():
    """Argument validation comes before anything touches the device: no GPU needed."""
    import swimmer_amd as sw
    lib = sw._lib.load()
    one = ctypes.c_void_p(8)
    lean, packed, split = sw._lib.FLAG_CAPTURE_LEAN_V1, sw._lib.FLAG_CAPTURE_PACKED_V1, sw._lib.FLAG_CAPTURE_SPLIT
    for flags, want in ((lean, 3), (lean | packed, 4), (lean | split, 4), (lean | packed | split, 4), (32, 4), (64, 4), (256, 4),
                        (lean | sw._lib.FLAG_ROLLOUT_QUAD, 3)):
        p = sw.SwParams.make(3, flags=flags)
        # n_roll = -1: a valid parameter block gets as far as the size check (SW_ERR_SIZE = 3), no further
        assert lib.sw_rollout_f64(ctypes.byref(p), -1, 1, one, None, None, None, one, one, None, one, None,
                                  None) == want, flags


@pytest.fixture(scope="module")
def disassembly():
    return _disassemble()


def _steps(loop):
    """Steps per trip of a hot loop: every step has one range test."""
    return len([x for x in loop if x.startswith("v_cmp_gt_f64")])


def _per_step(loop):
    steps = _steps(loop)
    f64 = len([x for x in loop if "f64" in x.split()[0]])
    dpp = len([x for x in loop if x.startswith("v_mov_b32_dpp")])
    return steps, f64 / steps, dpp / steps, len(loop) / steps


@needs_tools
@pytest.mark.parametrize("new,lean", PAIRS)
def test_three_f64_fewer_two_dpp_more_one_fewer_in_all(disassembly, new, lean):
    """Both counts are over the hot loop alone: the re-normalisation blocks (.subsection 1) lie behind the kernel's
    last instruction, outside the loop's address range."""
    steps, f64, dpp, total = _per_step(_hot_loop(disassembly, new)[0])
    lsteps, lf64, ldpp, ltotal = _per_step(_hot_loop(disassembly, lean)[0])
    assert lsteps == LEAN_STEPS_PER_TRIP and steps in (8, 16)
    print(f"{new}: {steps} steps per trip; per step f64 {f64:.3f} (lean {lf64:.3f}), DPP moves {dpp:.3f} "
          f"(lean {ldpp:.3f}), all {total:.3f} (lean {ltotal:.3f}); per trip {total * steps:.0f} (lean "
          f"{ltotal * lsteps:.0f})")
    assert f64 <= lf64 - 3, (f64, lf64)
    assert dpp <= ldpp + 2, (dpp, ldpp)
    assert total <= ltotal - 1, (total, ltotal)


@needs_tools
@pytest.mark.parametrize("new,lean", PAIRS)
def test_one_store_per_step_no_load_no_scratch(disassembly, new, lean):
    loop, op = _hot_loop(disassembly, new)
    steps = _steps(loop)
    assert op.startswith("s_cbranch_scc")
    stores = [x for x in loop if re.match(r"(buffer|global|flat|scratch)_store", x)]
    assert len(stores) == steps and all(x.startswith("buffer_store_dwordx2") for x in stores), stores
    assert not [x for x in loop if re.match(r"(buffer|global|flat|scratch)_load", x)]
    banked = [x for x in loop if x.startswith("v_mov_b32_dpp") and "bank_mask:0xc" in x]
    assert len(banked) == 2 * steps, banked
    (sym, body), = _kernels(disassembly, new)
    assert not [x for x in body if x.startswith("scratch_")], (sym, "the kernel spills")


@needs_tools
@pytest.mark.parametrize("new,lean", PAIRS)
def test_range_test_still_branches_on_vcc(disassembly, new, lean):
    loop, _ = _hot_loop(disassembly, new)
    steps = _steps(loop)
    assert len([x for x in loop if x.startswith("s_cbranch_vccnz")]) == steps
    assert not [x for x in loop if x.startswith("s_cmp_lg_u64")]
    compares = [x for x in loop if x.startswith("v_cmp_gt_f64")]
    assert all(re.match(r"v_cmp_gt_f64_e64 vcc,", x) for x in compares), compares
    assert not [x for x in loop if re.match(r"s_\w+ (s\[\d+:\d+\], )?vcc\b", x) or re.match(r"s_mov_b64 vcc", x)]


@needs_tools
def test_the_lean_kernel_is_still_there(disassembly):
    for _, lean in PAIRS:
        loop, _ = _hot_loop(disassembly, lean)
        assert _steps(loop) == LEAN_STEPS_PER_TRIP


@pytest.mark.perf_lint
@needs_tools
def test_hot_loop_sits_where_the_sweep_put_it(disassembly):
    if PINNED_COMPILER not in _compiler():
        pytest.skip(f"the placement belongs to hipcc {PINNED_COMPILER}; another compiler lays the loop out anew")
    moved = []
    for fragment, (body, where) in EXPECTED.items():
        all_loops = _backward_loops(disassembly, fragment)
        loops = [(h, b) for h, b, op in all_loops if b == body and op.startswith("s_cbranch_scc")]
        if len(loops) != 1:
            biggest = max(all_loops, key=lambda t: t[1], default=None)
            moved.append(f"{fragment}: no hot loop of {body} bytes any more; largest backward loop now: "
                         f"{biggest and (biggest[1], biggest[0] % 64)}")
        elif loops[0][0] % 64 != where:
            moved.append(f"{fragment}: hot loop ({body} bytes) at offset {loops[0][0] % 64}, the sweep chose {where}")
    assert not moved, ("re-run the pad sweep (-DSW_OCTS_LOOP_PAD=k) and update EXPECTED:\n  " + "\n  ".join(moved))
