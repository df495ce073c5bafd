"""Safe exploration with CACLA on easy parameterised LQR problems: the mirror of the reference's
cacla/cacla_safe_agent.py.  An action is tried on the simulator first and taken in the real environment only when the
simulator's next state keeps the cost under a threshold lowered by the simulator's error.

`Constraint` is the safety constraint on the state; CACLA_LQR_SE_agent computes the simulator threshold at every step
(unbounded spaces), CACLA_LQR_SE_fix uses one threshold for the run, CACLA_Bounded_LQR_SE_agent derives it from the
bounds of the spaces and CACLA_AffineQR_SE_agent from the affine problem's constant.  Their run() loops are the
reference's, on the fused kernel (sw_lqr_cacla_run_f64, cacla/lqr.py).

Returned arrays are the reference's: a refused step repeats the last entry, refused steps before the first admitted
one add nothing (the arrays are then shorter than n_iter; np.array([]) when nothing was ever admitted).  After run():
admitted, violations (admitted steps whose real next state broke the constraint: the reference prints a line for
each, here they are counted), actor_updates, status.
"""
import numpy as np

from . import lqr
from .cacla_agent import CACLA_LQR_agent
from .lqr import norm_cost  # noqa: F401


class Constraint():
    """A safety constraint on the state: cost(state) <= l, with L_c the Lipschitz constant of the cost.  cost:
    lqr.norm_cost(np.inf | 2 | 1), or a callable equal to one of these norms (lqr.cost_code)."""

    def __init__(self, cost, l, L_c):
        self.cost = cost
        self.l = l
        self.L_c = L_c

    def satisfied(self, state):
        return self.cost(state) <= self.l


class CACLA_LQR_SE_agent(CACLA_LQR_agent):
    """Safe exploration without bounds on state and action: the simulator threshold of every step is
    l - epsilon L_c (op_norm_der_A ||state||_2 + op_norm_der_B ||action||_2)."""

    def __init__(self, real_env, simulator, epsilon, constraint):
        super(CACLA_LQR_SE_agent, self).__init__(real_env)
        self.simulator = simulator
        self.constraint = constraint
        self.epsilon = epsilon
        lqr.cost_code(constraint.cost, self.F.shape[1])          # an unsupported cost fails here, not in run()

    def compute_sim_threshold(self, L_c, epsilon, state, action):
        L_theta = (self.simulator.op_norm_der_A * np.linalg.norm(state, 2)
                   + self.simulator.op_norm_der_B * np.linalg.norm(action, 2))
        return self.constraint.l - epsilon * L_c * L_theta

    def run(self, n_iter, gamma, alpha, sigma, H=1000):
        return lqr.run_single(self, "se", n_iter, gamma, alpha, sigma, H, self.simulator, self.epsilon,
                              self.constraint)


class CACLA_LQR_SE_fix(CACLA_LQR_SE_agent):
    """Safe exploration with the same Lipschitz constant L_theta, hence one simulator threshold, at every step."""

    def __init__(self, real_env, simulator, epsilon, constraint):
        super().__init__(real_env, simulator, epsilon, constraint)

    def set_simulator_threshold(self, L_theta):
        self.sim_threshold = self.constraint.l - self.epsilon * self.constraint.L_c * L_theta

    def run(self, n_iter, gamma, alpha, sigma, H=1000):
        return lqr.run_single(self, "fix", n_iter, gamma, alpha, sigma, H, self.simulator, self.epsilon,
                              self.constraint, threshold=self.sim_threshold)


class CACLA_Bounded_LQR_SE_agent(CACLA_LQR_SE_fix):
    """Bounded state and / or action spaces: L_theta from the bounds (BoundedEasyLinearQuadReg and its kin)."""

    def __init__(self, real_env, simulator, epsilon, constraint):
        super().__init__(real_env, simulator, epsilon, constraint)
        self.simulator = simulator
        n_obs = real_env.observation_space.shape[0]
        n_ac = real_env.action_space.shape[0]
        L_theta = (self.simulator.op_norm_der_A * np.sqrt(n_obs) * real_env.max_s
                   + self.simulator.op_norm_der_B * np.sqrt(n_ac) * real_env.max_a)
        self.set_simulator_threshold(L_theta)


class CACLA_AffineQR_SE_agent(CACLA_LQR_SE_fix):
    """The affine quadratic regulator (EasyAffineQuadReg), unbounded: L_theta = ||(0.1, 0)||."""

    def __init__(self, real_env, sim_env, epsilon, constraint):
        super(CACLA_AffineQR_SE_agent, self).__init__(real_env, sim_env, epsilon, constraint)
        L_theta = np.linalg.norm(np.array([0.1, 0]))
        self.set_simulator_threshold(L_theta)
