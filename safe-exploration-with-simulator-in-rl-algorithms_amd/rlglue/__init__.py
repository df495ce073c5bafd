"""The reference's RL-Glue experiment (rlglue/): SwimmerARSAgent on the native swimmer, whole runs in one launch."""
from .parameters import Parameters  # noqa: F401
from .experiment import SwimmerExperiment, SwimmerExperimentBatch  # noqa: F401
