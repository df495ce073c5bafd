"""Mirror of the reference's `cacla` package for the swimmer (cacla/cacla_agent.py, cacla/swimmer_experiment.py):
`CACLA_agent` with the reference's signature, `CACLABatch` for many independent agents in one launch per chunk of
steps, and the hyper-parameter grid of swimmer_experiment.py without Ray -- all on the fused kernel behind
sw_cacla_run_f64 (one wave per agent, the networks in registers, whole runs in one launch)."""
from . import swimmer_experiment  # noqa: F401
from .cacla_agent import CACLA_agent, CACLABatch, draw_networks, net_doubles, pack_net, unpack_net  # noqa: F401
