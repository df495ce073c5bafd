"""Build recipe for csrc/libswimmer_hip.so (hipcc, gfx950 only, in-tree): one object per source file, compiled in
parallel, linked once; and the one recipe for reading the built machine code back (disassemble)."""
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("SWIMMER_HIP_LIB") or os.path.join(CSRC, "libswimmer_hip.so")  # override: experiments
OBJ_DIR = LIB_PATH + ".obj"    # a library's objects live next to it: A/B builds (SWIMMER_HIP_LIB) never mix theirs
# the translation units: swimmer_kernels.hip includes the kernel families' files (FAMILIES; its header says why
# they have to be compiled together), swimmer_abi.hip is the rollout entry points and the ARS pipeline,
# swimmer_cacla.hip CACLA on the swimmer (a unit of its own: nothing in it is shared with the families),
# swimmer_cacla_safe.hip the same behind the simulator gate (likewise; the learner both run is swimmer_cacla_learner.h),
# swimmer_cacla_ensemble.hip the gate in an ensemble of simulators, the members in the wave's lanes (likewise; the one
# kernel body, argument check and launch of these two is swimmer_cacla_gated.h, each unit instantiating its own seven),
# swimmer_lqr.hip CACLA on the LQR problems (a unit of its own as well), swimmer_rlglue_ars.hip the RL-Glue ARS
# experiment on the twin model (likewise), swimmer_safe_ars_ensemble.hip the safe-ARS rollouts gated on an ensemble of
# simulators (likewise; its body is swimmer_rollout_safe_lane.inc)
SOURCES = ["swimmer_kernels.hip", "swimmer_abi.hip", "swimmer_cacla.hip", "swimmer_lqr.hip", "swimmer_cacla_safe.hip",
           "swimmer_cacla_ensemble.hip", "swimmer_rlglue_ars.hip", "swimmer_safe_ars_ensemble.hip", "direct_comm.cpp",
           "host_rng.cpp"]
FAMILIES = ["swimmer_rollout_row.hip", "swimmer_rollout_n3.hip", "swimmer_rollout_lane.hip",
            "swimmer_rollout_safe_multi.hip", "swimmer_step.hip", "swimmer_cov.hip", "swimmer_update.hip"]
HOST_ONLY = {"host_rng.cpp"}   # plain C++, no device pass: it picks its vector width from the CPU's features at
                               # run time (x86 builtins the device pass of a HIP compile refuses)
HEADERS = ["rlglue_env.cpp", os.path.join("..", "..", "include", "rlglue_swimmer.h"),
           "swimmer_launch.h", "swimmer_cov.h", "swimmer_device.h", "swimmer_rollout_lane.inc",
           "swimmer_rollout_quad3.inc", "swimmer_rollout_oct3.inc", "swimmer_rollout_octp3.inc",
           "swimmer_rollout_row.inc", "swimmer_rollout_multi.inc", "swimmer_rollout_safe_oct3.inc",
           "swimmer_rollout_safe_lane.inc", "swimmer_rollout_safe_multi.inc", "swimmer_update.inc", "swimmer_quad3.h",
           "swimmer_oct3.h", "swimmer_row.h", "swimmer_row_fused.h", "swimmer_twin.h", "swimmer_cacla_learner.h",
           "swimmer_cacla_gated.h", os.path.join("..", "..", "include", "swimmer_hip.h")] + FAMILIES
HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC"] + os.environ.get("SWIMMER_HIPCC_EXTRA", "").split()
HOST_FLAGS = ["-O3", "-std=c++17", "-fPIC"]
LINK_LIBS = ["-ldl"]   # direct_comm.cpp resolves RCCL at run time
LLVM = "/opt/rocm/lib/llvm/bin"


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the swimmer HIP library cannot be built")
    return exe


def _newer_than(path, deps):
    """True if `path` is missing or older than one of `deps` (paths relative to csrc/)."""
    if not os.path.exists(path):
        return True
    t = os.path.getmtime(path)
    deps = [os.path.join(CSRC, d) for d in deps]
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def is_stale():
    return _newer_than(LIB_PATH, SOURCES + HEADERS)


RLGLUE_LIB_PATH = os.path.join(CSRC, "librlglue_swimmer_hip.so")


def _object(src):
    return os.path.join(OBJ_DIR, os.path.splitext(src)[0] + ".o")


def _compile(src, verbose):
    flags = HOST_FLAGS + ["-x", "c++"] if src in HOST_ONLY else HIPCC_FLAGS + ["-x", "hip"]
    cmd = [_hipcc()] + flags + ["-c", os.path.join(CSRC, src), "-o", _object(src)]
    if verbose:
        print(" ".join(cmd), flush=True)
    done = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    if done.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src} (exit {done.returncode}):\n{done.stderr}")
    if verbose and done.stderr:
        print(done.stderr, end="", flush=True)


def build_library(force=False, verbose=False):
    """Compile the HIP kernels + C ABI into csrc/libswimmer_hip.so for gfx950, and the
    RL-Glue environment plug-in (csrc/librlglue_swimmer_hip.so) on top of it.  force: every object anew;
    otherwise an object is recompiled when its source or any header is newer than it."""
    if not force and not is_stale() and os.path.exists(RLGLUE_LIB_PATH):
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)
    todo = [s for s in SOURCES if force or _newer_than(_object(s), [s] + HEADERS)]
    jobs = max(1, min(16, int(os.environ.get("MAX_JOBS", 16))))   # never the machine's core count: it may be shared
    with ThreadPoolExecutor(max_workers=jobs) as pool:
        for _ in pool.map(lambda s: _compile(s, verbose), todo):   # the first failing compile raises here
            pass
    cmd = ([_hipcc(), "-shared", "-fPIC", "--offload-arch=gfx950"] + [_object(s) for s in SOURCES]
           + LINK_LIBS + ["-o", LIB_PATH])
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd, cwd=CSRC)
    cmd = [_hipcc()] + HIPCC_FLAGS + ["-shared", os.path.join(CSRC, "rlglue_env.cpp"), "-L" + CSRC,
                                      "-lswimmer_hip", "-Wl,-rpath,$ORIGIN", "-o", RLGLUE_LIB_PATH]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd, cwd=CSRC)
    return LIB_PATH


def disassemble(lib=None, raw_insn=False):
    """`llvm-objdump -d --no-show-raw-insn` of EVERY gfx950 code object in the library, one after the other, as a
    list of lines (raw_insn: with the instructions' encodings).  Every device translation unit leaves its own offload bundle in the library's .hip_fatbin
    section; clang-offload-bundler reads one bundle per file, so the section is cut at the bundles' magic first."""
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib or LIB_PATH, fat],
                       check=True)
        with open(fat, "rb") as f:
            blob = f.read()
        starts, at = [], blob.find(magic)
        while at >= 0:
            starts.append(at)
            at = blob.find(magic, at + 1)
        for k, (a, b) in enumerate(zip(starts, starts[1:] + [len(blob)])):
            bundle, elf = os.path.join(tmp, f"bundle{k}.bin"), os.path.join(tmp, f"gfx950_{k}.elf")
            with open(bundle, "wb") as f:
                f.write(blob[a:b])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={bundle}", f"--output={elf}"],
                           check=True)
            objdump = [f"{LLVM}/llvm-objdump", "-d"] + ([] if raw_insn else ["--no-show-raw-insn"])
            lines += subprocess.run(objdump + [elf], check=True, capture_output=True, text=True).stdout.split("\n")
    return lines
