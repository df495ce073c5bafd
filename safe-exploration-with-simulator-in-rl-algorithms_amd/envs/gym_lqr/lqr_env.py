"""Infinite-horizon, discrete-time LQR environments: the mirror of the reference's envs/gym_lqr/lqr_env.py.

    x[k+1] = A x[k] + B u[k] (+ C),   reward = -(x[k+1]^T Q x[k+1] + u[k]^T R u[k])

Host NumPy on purpose: a 2 x 2 product does not go to a GPU.  The CACLA agents (swimmer_amd.cacla) never call
`step`; they read the matrices and bounds through model_of() and run whole training runs on the GPU
(sw_lqr_cacla_run_f64), after which `state` is the run's final state.  The classes are here for what the reference's
users do with them besides: stepping by hand, evaluating a learnt F, being handed to an agent.

Class names, constructor signatures and attributes are the reference's (no gym dependency: the spaces are the
declarative Box of envs/swimmer.py).  What an environment lacks is expressed as the reference's own "no bound" and
"no drift": max_s = max_a = 0, C = 0.
"""
import numpy as np

from ..swimmer import Box


def reset_inbound(x, M):
    """Bound the coordinates of x by M or -M, IN PLACE, as the reference codes it (lqr_env.py:80-93): M == 0 is no
    bound; otherwise |x_i| > M becomes |x_i| / x_i * M (so +-inf becomes NaN, and a negative M flips signs)."""
    if M != 0:
        with np.errstate(invalid="ignore", divide="ignore"):
            size = np.abs(x)
            out = size > M
            x[out] = size[out] / x[out] * M
    return x


class LinearQuadReg(object):
    """Basic LQR: A [n, n], B [n, m], Q [n, n], R [m, m]."""
    max_s = 0
    max_a = 0

    def __init__(self, A, B, Q, R):
        self.A = A
        self.B = B
        self.Q = Q
        self.R = R
        n_obs = A.shape[1]
        n_ac = B.shape[1]
        inf = 1000
        self.observation_space = Box(-inf, inf, (n_obs,))
        self.action_space = Box(-inf, inf, (n_ac,))

    def _drift(self):
        return getattr(self, "C", None)

    def step(self, action):
        action = np.array(action)
        action = reset_inbound(action, self.max_a)
        obs = self.A @ self.state + self.B @ action
        if self._drift() is not None:
            obs = obs + self.C
        obs = reset_inbound(obs, self.max_s)
        self.state = obs
        rew = - (self.state.transpose() @ self.Q @ self.state + action.transpose() @ self.R @ action)
        return obs, rew, False, {'action': action}

    def reset(self):
        self.state = np.random.rand(self.observation_space.shape[0])
        return self.state

    def set_state(self, state):
        self.state = state


class EasyParamLinearQuadReg(LinearQuadReg):
    """The toy problem for sim-to-real transfer: A and B are scaled by theta."""

    def __init__(self, theta):
        A = np.array([[0, 1], [1, 0]]) * theta
        B = np.array([[0], [1]]) * theta
        Q = np.array([[1, 0], [0, 1]])
        R = np.array([[1]])
        super().__init__(A, B, Q, R)
        self.op_norm_der_A = 1
        self.op_norm_der_B = 1


class BoundedEasyLinearQuadReg(EasyParamLinearQuadReg):
    """Bounded state and action spaces: |x_t| <= max_s, |u_t| <= max_a (0: no bound)."""

    def __init__(self, theta, max_s, max_a):
        super().__init__(theta)
        self.max_s = max_s
        self.max_a = max_a

    def reset_inbound(self, x, M):
        return reset_inbound(x, M)


class BoundedActionEasyLinearQuadReg(BoundedEasyLinearQuadReg):
    """Bounded action space only; A does not depend on theta."""

    def __init__(self, theta, max_a):
        super(BoundedActionEasyLinearQuadReg, self).__init__(theta, 0, max_a)
        self.A = np.array([[0, 1], [1, 0]])


class EasyAffineQuadReg(EasyParamLinearQuadReg):
    """Affine quadratic regulator x' = A x + B u + C(theta); A and B do not depend on theta, no bounds."""

    def __init__(self, theta):
        super(EasyAffineQuadReg, self).__init__(1)
        self.C = np.array([0.1, 0]) * theta


def model_of(env):
    """(A [ns, ns], B [ns, na], C [ns], max_s, max_a, Q [ns, ns], R [na, na]) of an environment as float64: what the
    kernel takes.  Works on anything with the reference's attributes (A, B, Q, R; optionally C, max_s, max_a)."""
    A = np.asarray(env.A, dtype=np.float64)
    B = np.asarray(env.B, dtype=np.float64)
    ns, na = A.shape[1], B.shape[1]
    if A.shape != (ns, ns) or B.shape != (ns, na):
        raise ValueError(f"A must be square and B have as many rows: got {A.shape} and {B.shape}")
    C = np.zeros(ns) if getattr(env, "C", None) is None else np.asarray(env.C, dtype=np.float64).reshape(ns)
    Q = np.asarray(env.Q, dtype=np.float64).reshape(ns, ns)
    R = np.asarray(env.R, dtype=np.float64).reshape(na, na)
    return A, B, C, float(getattr(env, "max_s", 0)), float(getattr(env, "max_a", 0)), Q, R
