"""Mirror of the reference's `safe_ars` package for the hot path's batched one-step consumers:
`Basic_ARS` and `Safe_ARS` of safe_ars/ars.py on top of the HIP step kernel; `ARSBatch` trains many of them as one batch (one rollout launch with the gate inside
and one update launch per iteration), and `experiment` is safe_ars/experiment.py on top of it."""
from .ars import AbsObs, Basic_ARS, MaxAbsThetaDot, NativeCost, Safe_ARS  # noqa: F401
from .batch import ARSBatch  # noqa: F401
from . import experiment  # noqa: F401
