"""The reference's LQR environments (envs/gym_lqr/lqr_env.py)."""
from .lqr_env import (BoundedActionEasyLinearQuadReg, BoundedEasyLinearQuadReg, EasyAffineQuadReg,  # noqa: F401
                      EasyParamLinearQuadReg, LinearQuadReg)
