"""Time the REFERENCE's own LQR agents (NumPy, cacla/cacla_agent.py CACLA_LQR_agent and cacla/cacla_safe_agent.py) where
the reference is available -- it does not travel to the GPU machine: microseconds per step of the plain agent on the
sweep's instance and of the safe agent of safe_exploration_lqr.py, one process.  Quote the figure with its machine."""
import contextlib, importlib.util, io, os, sys, time
import numpy as np

spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "make_golden.py"))
mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
import cacla.cacla_agent as ref_agent  # noqa: E402  (reference modules)
import cacla.cacla_safe_agent as ref_safe  # noqa: E402
import envs.gym_lqr.lqr_env as ref_envs  # noqa: E402

STEPS = 20000


def plain():
    env = ref_envs.LinearQuadReg(np.array([[0, 1], [1, 0]]), np.array([[0], [1]]), np.array([[1, 0], [0, 1]]), np.array([[1]]))
    return ref_agent.CACLA_LQR_agent(env)


def safe():
    con = ref_safe.Constraint(lambda x: np.linalg.norm(x, np.inf), 4, 1)
    return ref_safe.CACLA_AffineQR_SE_agent(ref_envs.EasyAffineQuadReg(1.0), ref_envs.EasyAffineQuadReg(0.99), 0.01, con)


for name, make in (("CACLA_LQR_agent (lqr_2)", plain), ("CACLA_AffineQR_SE_agent", safe)):
    times = []
    for rep in range(3):
        np.random.seed(rep)
        agent = make()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            agent.run(STEPS, 1, 0.0001, 0.1)
        times.append((time.perf_counter() - t0) / STEPS)
    med = sorted(times)[1]
    print(f"{name}: {med * 1e6:.1f} us per step (median of 3 runs of {STEPS} steps; min {min(times) * 1e6:.1f}, "
          f"max {max(times) * 1e6:.1f}); lqr_experiment.py's 9 x 200 000 steps: {med * 1.8e6:.0f} s, "
          f"safe_exploration_lqr.py's 2 x 20 000: {med * 4e4:.1f} s")
print(f"{os.cpu_count()} logical CPUs here; /proc/cpuinfo:", next((l.split(':')[1].strip() for l in open('/proc/cpuinfo') if l.startswith('model name')), '?'))
