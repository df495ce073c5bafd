"""The built machine code of rollout_octp3_kernel, the packed record form of the n = 3 mirror-quad rollout with capture
and V2 moments (csrc/swimmer_rollout_octp3.inc), read out of the library's gfx950 code objects (no GPU needed).

* What the form is for: ONE trajectory store per env-step in the hot loop (the three-store kernel has three), and the
  two `v_mov_b32_dpp ... bank_mask:0xc` per step that put quad A's thetadot onto the B lanes.
* The kernel carries the riding covariance tile like its sibling: the ticket contract of test_isa_contracts.py holds.
* Where the hot loop sits in its 64-byte line (perf lint, one compiler build: see test_loop_placement.py)."""
import os
import re
import shutil

import pytest

from test_isa_contracts import _kernels
from test_loop_placement import LIB, LLVM, PINNED_COMPILER, ROOT, _backward_loops, _compiler, _disassemble

needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and shutil.which(f"{LLVM}/llvm-objdump")),
                                 reason="needs the built library and the ROCm llvm tools")

PACKED = ["rollout_octp3_kernelILb1E", "rollout_octp3_kernelILb0E"]   # ARS form, plain form
STEPS_PER_TRIP = 8
# (bytes of the hot loop's body, offset of its head inside a 64-byte line): the choice of the sweep over all sixteen
# offsets, profiles/r06_b_octp_pad_sweep.log
EXPECTED = {"rollout_octp3_kernelILb1E": (5772, 52), "rollout_octp3_kernelILb0E": (5772, 52)}   # pad 4


def test_flag_and_name():
    import swimmer_amd as sw
    assert sw._lib.FLAG_CAPTURE_SPLIT == 8 and sw._lib.kernel_flags("split") == 8
    flags = (sw._lib.FLAG_ROLLOUT_LANE, sw._lib.FLAG_ROLLOUT_QUAD, sw._lib.FLAG_MODEL_TWIN, sw._lib.FLAG_CAPTURE_SPLIT)
    assert len(set(flags)) == 4 and all(f & (f - 1) == 0 for f in flags)
    header = open(os.path.join(ROOT, "include", "swimmer_hip.h")).read()
    assert re.search(r"#define\s+SW_FLAG_CAPTURE_SPLIT\s+8\b", header)
    with pytest.raises(sw.SwimmerHipError):
        sw._lib.kernel_flags("packed")


def _hot_loop(lines, fragment):
    """The instructions of the kernel's largest backward loop (a loop's back edge is a conditional scalar branch; the
    unconditional backward branches are the returns from the out-of-line re-normalisation blocks)."""
    (sym, body), = _kernels(lines, fragment)
    start = next(i for i, l in enumerate(lines) if fragment in l and l.endswith(">:"))
    base = int(lines[start].split()[0], 16)
    head, size, op = max((t for t in _backward_loops(lines, fragment) if t[2].startswith("s_cbranch_scc")),
                         key=lambda t: t[1])
    text = []
    for l in lines[start + 1:]:
        if l.startswith("0000"):
            break
        m = re.match(r"\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", l)
        if m and head <= int(m.group(2), 16) < head + size + 4:
            text.append(m.group(1))
    assert base <= head
    return text, op


@pytest.fixture(scope="module")
def disassembly():
    return _disassemble()


@needs_tools
@pytest.mark.parametrize("fragment", PACKED)
def test_one_trajectory_store_per_step(disassembly, fragment):
    loop, op = _hot_loop(disassembly, fragment)
    assert op == "s_cbranch_scc0"
    stores = [x for x in loop if re.match(r"(buffer|global|flat|scratch)_store", x)]
    assert len(stores) == STEPS_PER_TRIP and all(x.startswith("buffer_store_dwordx2") for x in stores), stores
    assert not [x for x in loop if re.match(r"(buffer|global|flat|scratch)_load", x)]


@needs_tools
@pytest.mark.parametrize("fragment", PACKED)
def test_two_banked_dpp_moves_per_step(disassembly, fragment):
    loop, _ = _hot_loop(disassembly, fragment)
    banked = [x for x in loop if x.startswith("v_mov_b32_dpp") and "bank_mask:0xc" in x]
    assert len(banked) == 2 * STEPS_PER_TRIP, banked
    assert all("row_ror:8" in x and "bound_ctrl" not in x for x in banked), banked


@needs_tools
def test_the_three_store_kernel_is_still_there(disassembly):
    """FLAG_CAPTURE_SPLIT's kernel: three stores per step, for the A/B and the bit-identity tests."""
    loop, _ = _hot_loop(disassembly, "rollout_oct3_kernelILb1ELb1ELb1E")
    assert len([x for x in loop if x.startswith("buffer_store_dwordx2")]) == 3 * STEPS_PER_TRIP


@needs_tools
@pytest.mark.parametrize("fragment", PACKED)
def test_ticket_is_taken_after_the_tile_rows_stores_have_completed(disassembly, fragment):
    """test_isa_contracts.py's contract for the covariance tile that rides along in this kernel too."""
    ks = _kernels(disassembly, fragment)
    assert len(ks) == 1, (fragment, "not in the library")
    sym, body = ks[0]
    tickets = [i for i, x in enumerate(body) if re.match(r"global_atomic_add(_u32)?\s", x)]
    assert len(tickets) == 1, (sym, "expected exactly one ticket atomic", tickets)
    i = tickets[0]
    stores = [j for j in range(i) if re.match(r"(global|buffer|flat)_store", body[j])]
    assert stores, (sym, "no store ahead of the ticket?")
    between = body[stores[-1] + 1:i]
    assert any(x.startswith("s_waitcnt") and "vmcnt(0)" in x for x in between), \
        (sym, "no s_waitcnt vmcnt(0) between the tile row's last store and the ticket", between[-12:])
    assert any(x.startswith("s_barrier") for x in between), (sym, "the waves must meet before the ticket")


@pytest.mark.perf_lint
@needs_tools
def test_packed_hot_loop_sits_where_the_sweep_put_it(disassembly):
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
    assert not moved, ("re-run the pad sweep (-DSW_OCTP_LOOP_PAD=k) and update EXPECTED:\n  " + "\n  ".join(moved))
