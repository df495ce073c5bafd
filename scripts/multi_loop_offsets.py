"""Where the hot loops of the multi-agent rollout kernels (ars_multi_*_kernel, and the safe batch's
ars_gate_multi_*_kernel and ars_counted_*_kernel) sit in their 64-byte code line, next to
their single-agent twins (the form's ARS kernel without capture, same n, same MOM), from the built library (no GPU).

    python scripts/multi_loop_offsets.py

One line per pair: bytes and offset of the hot loop of both kernels, whether the loops hold the same instructions
(opcode counts), and the pad that would move the multi loop to its twin's offset (csrc/swimmer_launch.h,
*_multi_loop_pad: run again after changing what lies between a pin and its loop)."""
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import swimmer_amd  # noqa: E402

PAIRS = [("ars_multi_oct3_kernelILb1E", "rollout_oct3_kernelILb1ELb0ELb1E", 0),
         ("ars_multi_oct3_kernelILb0E", "rollout_oct3_kernelILb1ELb0ELb0E", 0),
         ("ars_multi_quad3_kernelILb1E", "rollout_quad3_kernelILb1ELb0ELb1E", 0),
         ("ars_multi_quad3_kernelILb0E", "rollout_quad3_kernelILb1ELb0ELb0E", 0)]
# the row kernel's hot loop is the one-step loop inside a trip: the second largest back edge
PAIRS += [(f"ars_multi_row_kernelILi{n}ELb{mom}E", f"rollout_row_kernelILi{n}ELb1ELb0ELb{mom}E", 1)
          for n in range(4, 9) for mom in (1, 0)]
# the safe batch: the multi-agent gate kernels next to the form's single-agent gate kernel, the counted multi-agent
# rollout kernels next to the form's ARS kernel without capture (csrc/swimmer_launch.h, *_gate_multi_loop_pad and
# *_counted_loop_pad)
PAIRS += [("ars_gate_multi_oct3_kernel", "ars_gate_oct3_kernel", 0),
          ("ars_gate_multi_quad3_kernel", "ars_gate_quad3_kernel", 0)]
PAIRS += [(f"ars_gate_multi_row_kernelILi{n}E", f"ars_gate_row_kernelILi{n}E", 1) for n in range(4, 9)]
PAIRS += [(f"ars_counted_oct3_kernelILb{mom}E", f"rollout_oct3_kernelILb1ELb0ELb{mom}E", 0) for mom in (1, 0)]
PAIRS += [(f"ars_counted_quad3_kernelILb{mom}E", f"rollout_quad3_kernelILb1ELb0ELb{mom}E", 0) for mom in (1, 0)]
PAIRS += [(f"ars_counted_row_kernelILi{n}ELb{mom}E", f"rollout_row_kernelILi{n}ELb1ELb0ELb{mom}E", 1)
          for n in range(4, 9) for mom in (1, 0)]

# the ensemble gate's member kernels next to the form's multi-agent gate kernel (*_gate_ens_loop_pad)
PAIRS += [("ars_gate_ens_oct3_kernel", "ars_gate_multi_oct3_kernel", 0),
          ("ars_gate_ens_quad3_kernel", "ars_gate_multi_quad3_kernel", 0)]
PAIRS += [(f"ars_gate_ens_row_kernelILi{n}E", f"ars_gate_multi_row_kernelILi{n}E", 1) for n in range(4, 9)]


def kernel(lines, fragment):
    start = next(i for i, l in enumerate(lines) if fragment in l and l.endswith(">:"))
    out = []
    for l in lines[start + 1:]:
        if l.startswith("0000"):
            break
        m = re.match(r"\s+(\S+)(.*?)\s*//\s*([0-9A-Fa-f]+):", l)
        if m:
            out.append((int(m.group(3), 16), m.group(1), m.group(2)))
    return out


def hot_loop(body, which, like=None):
    """(head address, bytes, opcode counts) of the `which`-th largest loop closed by s_cbranch_scc0, or, with `like`,
    of the loop closest to `like` bytes (the twins also hold loops the multi kernels have no use for)."""
    loops = []
    for addr, op, rest in body:
        if op == "s_cbranch_scc0":
            off = int(rest.split()[0])
            if off >= 32768:
                loops.append((4 * (65536 - off), addr + 4 - 4 * (65536 - off)))
    loops.sort(reverse=True)
    size, head = loops[which] if like is None else min(loops, key=lambda t: abs(t[0] - like))
    return head, size, collections.Counter(op for a, op, _ in body if head <= a < head + size)


def main():
    lines = swimmer_amd._build.disassemble()
    for multi, single, which in PAIRS:
        hm, bm, cm = hot_loop(kernel(lines, multi), which)
        hs, bs, cs = hot_loop(kernel(lines, single), which, like=bm)
        diff = {k: (cs[k], cm[k]) for k in set(cm) | set(cs) if cm[k] != cs[k]}
        print(f"{multi:36s} {bm:5d} bytes at {hm % 64:2d} | twin {bs:5d} bytes at {hs % 64:2d} | "
              f"pad {((hs - hm) % 64) // 4:+d} (mod 16) | opcode counts {'equal' if not diff else diff}")


if __name__ == "__main__":
    main()
