"""Mirror of the reference's `cacla` package.

Swimmer (cacla/cacla_agent.py, cacla/swimmer_experiment.py): `CACLA_agent` with the reference's signature,
`CACLABatch` for many independent agents in one launch per chunk of steps, and the hyper-parameter grid of
swimmer_experiment.py without Ray -- all on the fused kernel behind sw_cacla_run_f64 (one wave per agent, the networks
in registers, whole runs in one launch).

Swimmer with safe exploration (the combination the reference stops short of): `CACLA_SE_agent`, `CACLA_SE_Batch`
and `swimmer_experiment.safe_compare` -- the same learner behind a per-step simulator gate, on the fused kernel behind
sw_cacla_safe_run_f64.  With `sim_ensemble=` / `sim_ensembles=`, and in `swimmer_experiment.safe_compare_ensemble`, the
gate runs in an ensemble of up to 64 simulators per agent, the members in the lanes of the agent's wave
(sw_cacla_safe_ensemble_run_f64), and a step is taken only where every member admits it.

LQR (cacla/cacla_agent.py:202-297, cacla/cacla_safe_agent.py, cacla/lqr_experiment.py,
cacla/safe_exploration_lqr.py, cacla/window.py): `CACLA_LQR_agent`, the safe agents of `cacla_safe_agent`,
`CACLA_LQR_Batch` for many independent agents, and the two experiment scripts as functions -- on the fused kernel
behind sw_lqr_cacla_run_f64 (one agent per lane)."""
from . import swimmer_experiment  # noqa: F401
from .cacla_agent import (CACLA_agent, CACLA_LQR_agent, CACLABatch, draw_networks, net_doubles, pack_net,  # noqa: F401
                          unpack_net)
from .cacla_safe_swimmer import CACLA_SE_agent, CACLA_SE_Batch, trim_rewards  # noqa: F401
from .lqr import CACLA_LQR_Batch, norm_cost  # noqa: F401
from .cacla_safe_agent import (CACLA_AffineQR_SE_agent, CACLA_Bounded_LQR_SE_agent, CACLA_LQR_SE_agent,  # noqa: F401
                               CACLA_LQR_SE_fix, Constraint)
from .window import window_convolution  # noqa: F401
from . import lqr_experiment, safe_exploration_lqr  # noqa: F401
