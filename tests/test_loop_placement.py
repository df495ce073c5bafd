"""Where the rollout kernels' hot loops sit inside their 64-byte code line (csrc/swimmer_launch.h,
SW_PIN_LOOP).  A lone wave's issue rate depends on it -- the same instructions ran 3.5 % (n = 3) to 11 %
(n = 7) apart at different offsets -- and the offset of an unpinned loop moves with every unrelated edit
earlier in the file.  This test reads the offsets out of the built library and compares them with the ones
the sweep on the GPU chose (profiles/r03_p_loop_pad_sweep_*.log, r03_q_final_pads.log).  If it fails after
a change to a kernel (or a new compiler), the loop has moved relative to its pin: run the sweep again
(scripts/ab_probe.sh over builds with -DSW_OCT_LOOP_PAD=k -DSW_QUAD_LOOP_PAD=k -DSW_ROW_LOOP_PAD=k) and
update the pads and this table.

A PERF LINT, not a correctness test (marker `perf_lint`: deselect with -m "not perf_lint"): the table belongs to
ONE compiler build (PINNED_COMPILER) -- under any other hipcc the test skips, because its offsets mean nothing
there -- and a failure lists every loop's new (bytes, offset), so updating the table after a deliberate kernel
change is mechanical."""
import os
import re
import shutil
import subprocess

import pytest

import swimmer_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "safe-exploration-with-simulator-in-rl-algorithms_amd", "csrc", "libswimmer_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"

PINNED_COMPILER = "roc-7.2.0 26014"      # `hipcc --version`: the build the sweep's offsets belong to

# kernel (mangled-name fragment) -> (bytes of the hot loop's body, offset of its head inside a 64-byte line)
EXPECTED = {
    "rollout_oct3_kernelILb1ELb1ELb1E": (5840, 56),     # eight steps per trip; 56 = the 0.2245 ms point of the sweep
    "rollout_oct3_kernelILb1ELb0ELb1E": (5588, 28),     # V2 without capture
    "rollout_oct3_kernelILb1ELb0ELb0E": (5236, 0),      # V1 without capture
    "rollout_oct3_kernelILb1ELb1ELb0E": (5548, 40),     # V1 with capture
    "rollout_row_kernelILi4ELb1ELb1ELb1E": (1200, 0),
    "rollout_row_kernelILi5ELb1ELb1ELb1E": (1468, 32),
    "rollout_row_kernelILi6ELb1ELb1ELb1E": (1752, 28),
    "rollout_row_kernelILi6ELb1ELb0ELb1E": (1712, 4),
    "rollout_row_kernelILi6ELb1ELb0ELb0E": (1676, 4),
    "rollout_row_kernelILi6ELb1ELb1ELb0E": (1712, 56),
    "rollout_row_kernelILi7ELb1ELb1ELb1E": (2048, 0),
    "rollout_row_kernelILi8ELb1ELb1ELb1E": (2452, 56),
}


def _disassemble():
    """The disassembly of every gfx950 code object in the library (the one recipe: swimmer_amd._build.disassemble)."""
    return swimmer_amd._build.disassemble(LIB)


def _backward_loops(lines, fragment):
    """(head address, body bytes, branch mnemonic) of every backward branch of the kernel."""
    start = next(i for i, l in enumerate(lines) if fragment in l and l.endswith(">:"))
    out = []
    for l in lines[start + 1:]:
        if l.startswith("0000"):
            break
        m = re.match(r"\s+(s_c?branch\w*)\s+(\d+)\s.*//\s*([0-9A-Fa-f]+):", l)
        if not m:
            continue
        off, addr = int(m.group(2)), int(m.group(3), 16)
        if off >= 32768:
            off -= 65536
            out.append((addr + 4 + 4 * off, -4 * off, m.group(1)))
    return out


def _compiler():
    try:
        return subprocess.run([shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "--version"], capture_output=True,
                              text=True, timeout=60).stdout
    except OSError:
        return ""


@pytest.mark.perf_lint
@pytest.mark.skipif(not (os.path.exists(LIB) and shutil.which(f"{LLVM}/llvm-objdump")),
                    reason="needs the built library and the ROCm llvm tools")
def test_hot_loops_sit_where_the_sweep_put_them():
    if PINNED_COMPILER not in _compiler():
        pytest.skip(f"the placement table belongs to hipcc {PINNED_COMPILER}; another compiler lays the loops out anew")
    lines = _disassemble()
    moved = []
    for fragment, (body, where) in EXPECTED.items():
        all_loops = _backward_loops(lines, fragment)
        loops = [(h, b) for h, b, op in all_loops if b == body and op == "s_cbranch_scc0"]
        if len(loops) != 1:
            biggest = max(all_loops, key=lambda t: t[1], default=None)
            moved.append(f"{fragment}: no hot loop of {body} bytes any more (the kernel's code changed); largest "
                         f"backward loop now: {biggest and (biggest[1], biggest[0] % 64)}")
        elif loops[0][0] % 64 != where:
            moved.append(f"{fragment}: hot loop ({body} bytes) at offset {loops[0][0] % 64} of its 64-byte line, "
                         f"the sweep chose {where}")
    assert not moved, ("loops moved relative to their pins -- re-run the pad sweep and update EXPECTED "
                       "(new (bytes, offset) listed):\n  " + "\n  ".join(moved))
