from .swimmer import SwimmerEnv, VecSwimmerEnv, Box, register_kwargs  # noqa: F401
from . import gym_lqr  # noqa: F401
