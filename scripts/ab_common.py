"""What the same-box A/B scripts (cacla_ab.py, step_ab.py) have in common: two builds of libswimmer_hip.so, OLD and
NEW, compared in fresh child processes -- are the results the same bits, and is the kernel time the same.

    compare(description, script, children)    # the script's main(): OLD.so NEW.so [--rounds R] [--timeout S] [--log FILE]

Per round and library one fresh child per entry of `children` = ((name, extra environment), ...), with SWIMMER_HIP_LIB
set: `python SCRIPT --child DIR` under its own `timeout -k 10`, OLD's children, then NEW's, round after round, one
after another; nothing is retried, and the comparison stops at the first child that does not exit 0.  A child leaves
DIR/cases.npz (arrays) and, if it timed anything, DIR/times.json ({row: [ms, ...]}).

Every array of OLD is compared with NEW's by its bits (dtype, shape and bytes: a NaN equals only the same NaN), the
timings are printed side by side.  With R > 1 the spread of OLD's medians over the rounds is the noise floor: NEW's
median of every round has to lie at or below OLD's largest.  Exit status 1: arrays differ; 3: a time above the floor;
a child's own status if one failed (124: its time limit).

Build OLD in a `git worktree` of the parent commit; a library whose sources are newer than it is rebuilt by the test
suite's conftest (not by these scripts), so build it last or copy it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def compare(description, script, children=(("", {}),)):
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per child")
    ap.add_argument("--log", help="also write the report here")
    args = ap.parse_args()
    libs = {"OLD": os.path.abspath(args.old), "NEW": os.path.abspath(args.new)}
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def finish(rc):
        if args.log:
            with open(args.log, "w") as f:
                f.write("\n".join(lines) + "\n")
        sys.exit(rc)

    for tag, path in libs.items():
        if not os.path.exists(path):
            sys.exit(f"{tag}: {path} does not exist")
        say(f"{tag} = {path}")
    medians, differ = {"OLD": {}, "NEW": {}}, 0
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(args.rounds):
            got = {}
            for tag, path in libs.items():
                arrays, times = {}, {}
                for name, extra in children:
                    out = os.path.join(tmp, f"{tag}_{rnd}_{name}")
                    os.makedirs(out)
                    say(f"round {rnd + 1}, {tag}{' ' + name if name else ''}:")
                    rc = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable,
                                         os.path.abspath(script), "--child", out],
                                        env=dict(os.environ, SWIMMER_HIP_LIB=path, **extra)).returncode
                    if rc != 0:
                        say(f"{tag} child ended with status {rc}: stopping here")
                        finish(rc if rc > 0 else 128 - rc)
                    arrays.update({name + key: a for key, a in np.load(os.path.join(out, "cases.npz")).items()})
                    if os.path.exists(os.path.join(out, "times.json")):
                        with open(os.path.join(out, "times.json")) as f:
                            times.update(json.load(f))
                got[tag] = (arrays, times)
            (a_old, t_old), (a_new, t_new) = got["OLD"], got["NEW"]
            bad = [k for k in a_old if k not in a_new or not same_bits(a_old[k], a_new[k])]
            bad += [k for k in a_new if k not in a_old]
            differ += len(bad)
            say(f"round {rnd + 1}: {len(a_old) - len(bad)} of {len(a_old)} arrays bit-equal"
                + ("" if not bad else "; DIFFERENT: " + ", ".join(bad)))
            for key in t_old:
                o, n = t_old[key], t_new[key]
                medians["OLD"].setdefault(key, []).append(statistics.median(o))
                medians["NEW"].setdefault(key, []).append(statistics.median(n))
                say(f"  {key:<42} ms  OLD median {statistics.median(o):8.4f} ({min(o):.4f} .. {max(o):.4f})   "
                    f"NEW median {statistics.median(n):8.4f} ({min(n):.4f} .. {max(n):.4f})   "
                    f"NEW / OLD {statistics.median(n) / statistics.median(o):.4f}")
    above = 0
    if args.rounds > 1:
        say("over the rounds (ms): OLD's medians min .. max are the noise floor; NEW's medians must not exceed "
            "OLD's max")
        for key, o in medians["OLD"].items():
            n = medians["NEW"][key]
            ok = max(n) <= max(o)
            above += 0 if ok else 1
            say(f"  {key:<42} OLD {min(o):8.4f} .. {max(o):8.4f}   NEW {min(n):8.4f} .. {max(n):8.4f}   "
                + ("at or below" if ok else "ABOVE"))
    say("arrays: " + ("all bit-equal" if not differ else f"{differ} DIFFERENT"))
    finish(1 if differ else 3 if above else 0)
