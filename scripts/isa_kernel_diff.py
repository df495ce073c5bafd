"""Per-kernel comparison of the gfx950 machine code of two builds of libswimmer_hip.so (no GPU needed).

    python scripts/isa_kernel_diff.py OLD.so NEW.so

Prints every kernel of OLD whose instruction text differs in NEW (or is missing there), the kernels NEW adds, and a
count.  Absolute addresses are ignored; branch offsets and everything else of an instruction are compared."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import swimmer_amd  # noqa: E402


def kernels(lib):
    text = swimmer_amd._build.disassemble(lib)     # every gfx950 code object in the library
    out, cur = {}, None
    for line in text:
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"\s+(\S.*?)\s*//\s*[0-9A-Fa-f]+:", line)
        if m and cur is not None:
            cur.append(m.group(1))
    return out


def main(old, new):
    a, b = kernels(old), kernels(new)
    same = 0
    for name, body in a.items():
        if name not in b:
            print("missing :", name)
        elif b[name] != body:
            print("differs :", name, len(body), "->", len(b[name]), "instructions")
        else:
            same += 1
    added = [name for name in b if name not in a]
    for name in added:
        print("added   :", name)
    print(f"{same} of {len(a)} kernels identical, {len(added)} added")
    return 0 if same == len(a) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
