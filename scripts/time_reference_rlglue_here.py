"""Time the REFERENCE's own RL-Glue agent (rlglue/agent/SwimmerAgent.py) in the build container -- it cannot travel to
the GPU box: seconds per environment step at the shipped parameters.txt (n = 3, N = 1, H = 1000), driven by the
stand-in harness of tests/golden/make_rlglue_golden.py (in-memory codec modules, the CPU oracle's twin step in place of
the C++ environment).  It EXCLUDES the sockets: the reference runs agent, environment and experiment as three
processes around rl_glue, two round trips per step, which this harness does not have.  Container-only script; quote
the figure with its machine."""
import importlib.util
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("make_rlglue_golden",
                                              os.path.join(HERE, "..", "tests", "golden", "make_rlglue_golden.py"))
mk = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mk)

ITERATIONS = 3
times = []
for rep in range(3):
    t0 = time.perf_counter()
    mk.run_reference(rep, 3, 1, 1, 1000, 0.02, 0.02, 5.0, 0.01, ITERATIONS)
    times.append((time.perf_counter() - t0) / (ITERATIONS * 3 * 1000))
med = sorted(times)[1]
print(f"{med * 1e6:.1f} us per environment step (median of 3 runs of {ITERATIONS * 3000} steps; min {min(times) * 1e6:.1f}, "
      f"max {max(times) * 1e6:.1f}), sockets excluded; `./SwimmerExperiment 100000` at the shipped parameters is 3e8 "
      f"steps: {med * 3e8 / 3600:.1f} h in this harness")
print(f"{os.cpu_count()} logical CPUs here; /proc/cpuinfo:",
      next((l.split(':')[1].strip() for l in open('/proc/cpuinfo') if l.startswith('model name')), '?'))
