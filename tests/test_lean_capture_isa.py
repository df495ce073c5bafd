"""The built machine code of rollout_octl3_kernel, the lean mode of the packed record form of the n = 3 mirror-quad
rollout (csrc/swimmer_rollout_octp3.inc with SW_OCTP_LEAN 1), read out of the library's gfx950 code objects (no GPU
needed), and the flag that keeps a launch on the first packed kernel.

What the mode is for is fewer scalar instructions per trip of eight steps, with everything else as it was:
* the eight trajectory stores take their scalar offsets from loop-invariant registers: no chain of s_add behind them
  (the trip counter's adds are all that is left), and still one store per step and no load;
* the range test branches on vcc (eight s_cbranch_vccnz per trip), without the scalar compare of the lane mask;
* so the hot loop is at least 20 instructions shorter than rollout_octp3_kernel's IN THE SAME LIBRARY -- a relative
  count, which another compiler build does not break (pinned compiler: 863 against 884, the back edge included);
* the first packed kernel is still in the library (FLAG_CAPTURE_PACKED_V1, the A/B and the bit-identity tests).
Where the hot loop sits in its 64-byte line is a perf lint for one compiler build (see test_loop_placement.py)."""
import ctypes
import os
import re
import shutil

import pytest

from test_loop_placement import LIB, LLVM, PINNED_COMPILER, ROOT, _backward_loops, _compiler, _disassemble
from test_packed_capture_isa import _hot_loop

needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and shutil.which(f"{LLVM}/llvm-objdump")),
                                 reason="needs the built library and the ROCm llvm tools")

# (lean kernel, the packed kernel it is measured against): ARS form, plain form
LEAN = [("rollout_octl3_kernelILb1E", "rollout_octp3_kernelILb1E"),
        ("rollout_octl3_kernelILb0E", "rollout_octp3_kernelILb0E")]
STEPS_PER_TRIP = 8
# (bytes of the hot loop's body, offset of its head inside a 64-byte line): the choice of the sweep over the eight
# even pads, profiles/r08_b_octl_pad_sweep.log
EXPECTED = {"rollout_octl3_kernelILb1E": (5688, 0), "rollout_octl3_kernelILb0E": (5688, 0)}   # pad 2


def test_flag_and_name():
    import swimmer_amd as sw
    assert sw._lib.FLAG_CAPTURE_PACKED_V1 == 16 and sw._lib.kernel_flags("packed_v1") == 16
    assert sw._lib.kernel_flags("split") == sw._lib.FLAG_CAPTURE_SPLIT == 8 and sw._lib.kernel_flags("auto") == 0
    flags = (sw._lib.FLAG_ROLLOUT_LANE, sw._lib.FLAG_ROLLOUT_QUAD, sw._lib.FLAG_MODEL_TWIN, sw._lib.FLAG_CAPTURE_SPLIT,
             sw._lib.FLAG_CAPTURE_PACKED_V1)
    assert len(set(flags)) == 5 and all(f & (f - 1) == 0 for f in flags)
    header = open(os.path.join(ROOT, "include", "swimmer_hip.h")).read()
    assert re.search(r"#define\s+SW_FLAG_CAPTURE_PACKED_V1\s+16\b", header)
    assert re.search(r"#define\s+SW_ABI_VERSION\s+3\b", header) and sw._lib.ABI_VERSION == 3
    with pytest.raises(sw.SwimmerHipError):
        sw._lib.kernel_flags("packed")


def test_both_capture_flags_at_once_are_refused():
    """Argument validation comes before anything touches the device: no GPU needed."""
    import swimmer_amd as sw
    lib = sw._lib.load()
    one = ctypes.c_void_p(8)
    for flags, want in ((sw._lib.FLAG_CAPTURE_PACKED_V1, 3), (sw._lib.FLAG_CAPTURE_SPLIT, 3),
                        (sw._lib.FLAG_CAPTURE_PACKED_V1 | sw._lib.FLAG_CAPTURE_SPLIT, 4), (32, 4)):
        p = sw.SwParams.make(3, flags=flags)
        # n_roll = -1: a valid parameter block gets as far as the size check (SW_ERR_SIZE = 3), no further
        assert lib.sw_rollout_f64(ctypes.byref(p), -1, 1, one, None, None, None, one, one, None, one, None,
                                  None) == want, flags


@pytest.fixture(scope="module")
def disassembly():
    return _disassemble()


@needs_tools
@pytest.mark.parametrize("lean,packed", LEAN)
def test_one_store_per_step_and_no_load(disassembly, lean, packed):
    loop, op = _hot_loop(disassembly, lean)
    assert op == "s_cbranch_scc0"
    stores = [x for x in loop if re.match(r"(buffer|global|flat|scratch)_store", x)]
    assert len(stores) == STEPS_PER_TRIP and all(x.startswith("buffer_store_dwordx2") for x in stores), stores
    assert not [x for x in loop if re.match(r"(buffer|global|flat|scratch)_load", x)]
    banked = [x for x in loop if x.startswith("v_mov_b32_dpp") and "bank_mask:0xc" in x]
    assert len(banked) == 2 * STEPS_PER_TRIP, banked
    assert all("row_ror:8" in x and "bound_ctrl" not in x for x in banked), banked


@needs_tools
@pytest.mark.parametrize("lean,packed", LEAN)
def test_range_test_branches_on_vcc(disassembly, lean, packed):
    loop, _ = _hot_loop(disassembly, lean)
    assert len([x for x in loop if x.startswith("s_cbranch_vccnz")]) == STEPS_PER_TRIP
    assert not [x for x in loop if x.startswith("s_cmp_lg_u64")]
    compares = [x for x in loop if x.startswith("v_cmp_gt_f64")]
    assert len(compares) == STEPS_PER_TRIP and all(re.match(r"v_cmp_gt_f64_e64 vcc,", x) for x in compares), compares
    # nothing else in the loop may write vcc between a compare and its branch (the mask would have to be moved away)
    assert not [x for x in loop if re.match(r"s_\w+ (s\[\d+:\d+\], )?vcc\b", x) or re.match(r"s_mov_b64 vcc", x)]


@needs_tools
@pytest.mark.parametrize("lean,packed", LEAN)
def test_no_scalar_add_chain_behind_the_stores(disassembly, lean, packed):
    loop, _ = _hot_loop(disassembly, lean)
    adds = [x for x in loop if x.startswith("s_add")]
    assert len(adds) <= 3, adds
    # the stores' scalar offsets: seven registers and the inline constant 0
    soffsets = [re.match(r"buffer_store_dwordx2 v\[\d+:\d+\], v\d+, s\[\d+:\d+\], (\S+) offen", x)
                for x in loop if x.startswith("buffer_store_dwordx2")]
    assert all(soffsets), loop
    soffsets = [m.group(1) for m in soffsets]
    assert soffsets.count("0") == 1 and len(set(soffsets)) == STEPS_PER_TRIP, soffsets


@needs_tools
@pytest.mark.parametrize("lean,packed", LEAN)
def test_at_least_twenty_instructions_fewer_per_trip(disassembly, lean, packed):
    """Both counts are over the hot loop alone: the re-normalisation blocks (.subsection 1) lie behind the kernel's
    last instruction, outside the loop's address range."""
    n_lean, n_packed = len(_hot_loop(disassembly, lean)[0]), len(_hot_loop(disassembly, packed)[0])
    print(f"{lean}: {n_lean} instructions per trip, {packed}: {n_packed}")
    assert n_lean <= n_packed - 20, (n_lean, n_packed)


@needs_tools
def test_the_first_packed_kernel_is_still_there(disassembly):
    for _, packed in LEAN:
        loop, _ = _hot_loop(disassembly, packed)
        assert len([x for x in loop if x.startswith("s_cmp_lg_u64")]) == STEPS_PER_TRIP


@pytest.mark.perf_lint
@needs_tools
def test_lean_hot_loop_sits_where_the_sweep_put_it(disassembly):
    if PINNED_COMPILER not in _compiler():
        pytest.skip(f"the placement belongs to hipcc {PINNED_COMPILER}; another compiler lays the loop out anew")
    moved = []
    for fragment, (body, where) in EXPECTED.items():
        all_loops = _backward_loops(disassembly, fragment)
        loops = [(h, b) for h, b, op in all_loops if b == body and op == "s_cbranch_scc0"]
        if len(loops) != 1:
            biggest = max(all_loops, key=lambda t: t[1], default=None)
            moved.append(f"{fragment}: no hot loop of {body} bytes any more; largest backward loop now: "
                         f"{biggest and (biggest[1], biggest[0] % 64)}")
        elif loops[0][0] % 64 != where:
            moved.append(f"{fragment}: hot loop ({body} bytes) at offset {loops[0][0] % 64}, the sweep chose {where}")
    assert not moved, ("re-run the pad sweep (-DSW_OCTL_LOOP_PAD=k) and update EXPECTED:\n  " + "\n  ".join(moved))
