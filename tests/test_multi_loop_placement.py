"""Where the hot loops of the multi-agent mirror-quad kernels (sw_ars_rollouts_multi_f64, n = 3) sit in their 64-byte
code line: the offsets the pad sweep on the GPU chose (csrc/swimmer_launch.h oct_multi_loop_pad,
profiles/r05_multi_pad_sweep.log).  A perf lint like tests/test_loop_placement.py, tied to the same compiler build: a
failure means 'the loop moved relative to its pin, sweep again', not 'the results are wrong'."""
import os
import shutil

import pytest

from test_loop_placement import LIB, LLVM, PINNED_COMPILER, _backward_loops, _compiler, _disassemble

# kernel (mangled-name fragment) -> (bytes of the hot loop's body, offset of its head inside a 64-byte line)
EXPECTED = {
    "ars_multi_oct3_kernelILb1E": (5592, 24),     # V2: 198.2 us per launch, its single-agent twin 198.3
    "ars_multi_oct3_kernelILb0E": (5236, 0),      # V1: 188.3 us, twin 188.6
}


@pytest.mark.perf_lint
@pytest.mark.skipif(not (os.path.exists(LIB) and shutil.which(f"{LLVM}/llvm-objdump")),
                    reason="needs the built library and the ROCm llvm tools")
def test_multi_agent_hot_loops_sit_where_the_sweep_put_them():
    if PINNED_COMPILER not in _compiler():
        pytest.skip(f"the placement table belongs to hipcc {PINNED_COMPILER}; another compiler lays the loops out anew")
    lines = _disassemble()
    moved = []
    for fragment, (body, where) in EXPECTED.items():
        loops = [(h, b) for h, b, op in _backward_loops(lines, fragment) if b == body and op == "s_cbranch_scc0"]
        if len(loops) != 1:
            moved.append(f"{fragment}: no hot loop of {body} bytes any more: "
                         f"{sorted((b, h % 64) for h, b, _ in _backward_loops(lines, fragment))[-3:]}")
        elif loops[0][0] % 64 != where:
            moved.append(f"{fragment}: hot loop at offset {loops[0][0] % 64}, the sweep chose {where}")
    assert not moved, "re-run the pad sweep and update EXPECTED:\n  " + "\n  ".join(moved)
