from .parameters import EnvParam, ARSParam, Threshold  # noqa: F401
from .environment import Environment  # noqa: F401
from .ars_agent import ARSAgent  # noqa: F401
from .agent_batch import ARSAgentBatch  # noqa: F401
from .safe_agent_batch import SafeARSAgentBatch  # noqa: F401
from .experiment import Experiment  # noqa: F401
from .estimator_batch import EstimatorBatch  # noqa: F401
from . import safe_exploration  # noqa: F401
