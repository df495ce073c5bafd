"""MI355X-native implementation of the reference's swimmer-physics + ARS-rollout hot path.

Public surface (mirrors the reference's module layout for this path):
    envs.SwimmerEnv / envs.VecSwimmerEnv      envs/gym_swimmer/swimmer/remy_swimmer_env.py
    ars.Environment                           ars/environment.py
    ars.ARSAgent                              ars/ars_agent.py
    ars.Experiment                            ars/experiment.py  (its seeds train as one ars.ARSAgentBatch)
    ars.SafeARSAgentBatch / ars.safe_exploration.run   ars/safe_exploration.py  (every safe agent of the sweep in one batch)
    ars.EstimatorBatch                        ars/estimator.py  (many simulator estimates in lock-step, one launch per generation)
    ars.EnvParam / ars.ARSParam               ars/parameters.py
    safe_ars.Basic_ARS / safe_ars.Safe_ARS    safe_ars/ars.py  (batched one-step consumers of the step kernel)
    safe_ars.ARSBatch / safe_ars.experiment   safe_ars/experiment.py  (all seeds, basic and safe, as one training batch)
    cacla.CACLA_agent / cacla.CACLABatch      cacla/cacla_agent.py  (whole training runs in one fused launch)
    cacla.swimmer_experiment                  cacla/swimmer_experiment.py  (the whole grid as one batch)
    cacla.CACLA_LQR_agent, cacla.cacla_safe_agent.*, cacla.CACLA_LQR_Batch
                                              cacla/cacla_agent.py:202-297, cacla/cacla_safe_agent.py  (one agent per lane)
    envs.gym_lqr.lqr_env.*                    envs/gym_lqr/lqr_env.py  (host NumPy)
    cacla.lqr_experiment / cacla.safe_exploration_lqr / cacla.window
                                              cacla/lqr_experiment.py, cacla/safe_exploration_lqr.py, cacla/window.py
    rlglue.Parameters / rlglue.SwimmerExperiment / rlglue.SwimmerExperimentBatch
                                              rlglue/parameters.txt, rlglue/agent/SwimmerAgent.py under
                                              rlglue/experiment/SwimmerExperiment.cpp  (whole runs in one launch, twin model)
    kernels.*                                 thin wrappers of the C ABI (include/swimmer_hip.h)
"""
from . import _build, _lib, kernels  # noqa: F401
from ._lib import SwParams, SwimmerHipError  # noqa: F401
from .envs import SwimmerEnv, VecSwimmerEnv  # noqa: F401
from .ars import (ARSAgent, ARSAgentBatch, ARSParam, EnvParam, Environment, EstimatorBatch, Experiment,  # noqa: F401
                  SafeARSAgentBatch)
from . import safe_ars  # noqa: F401
from . import cacla  # noqa: F401
from . import rlglue  # noqa: F401

__all__ = ["SwParams", "SwimmerHipError", "SwimmerEnv", "VecSwimmerEnv", "ARSAgent", "ARSAgentBatch", "SafeARSAgentBatch", "ARSParam",
           "EnvParam", "Environment", "EstimatorBatch", "Experiment", "kernels"]
