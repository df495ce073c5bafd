"""Time the REFERENCE's own CACLA_agent.run (PyTorch autograd + NumPy swimmer, cacla/cacla_agent.py) in the build
container -- it cannot travel to the GPU box: seconds per agent-step at n = 3, one process, torch on one thread
and on its default thread count.  Container-only script; quote the figure with its machine."""
import contextlib, importlib.util, io, os, sys, time
import numpy as np
import torch

spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "make_golden.py"))
mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
import cacla.cacla_agent as ref  # noqa: E402  (reference module)

STEPS = 2000
for threads in (1, torch.get_num_threads()):
    torch.set_num_threads(threads)
    times = []
    for rep in range(3):
        torch.manual_seed(rep); np.random.seed(rep)
        env = mg.SwimmerEnv(n=3)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            ref.CACLA_agent(0.9, 0.01, 0.1).run(env, STEPS)
        times.append((time.perf_counter() - t0) / STEPS)
    print(f"torch threads {threads}: {sorted(times)[1] * 1e3:.3f} ms per agent-step (median of 3 runs of {STEPS} steps; "
          f"min {min(times) * 1e3:.3f}, max {max(times) * 1e3:.3f}); the grid's 960 x 10 000 agent-steps: "
          f"{sorted(times)[1] * 9.6e6 / 3600:.2f} h in one process")
print(f"{os.cpu_count()} logical CPUs here; /proc/cpuinfo:", next((l.split(':')[1].strip() for l in open('/proc/cpuinfo') if l.startswith('model name')), '?'))
