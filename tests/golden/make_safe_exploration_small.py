"""tests/golden/safe_exploration_small.npz: what ars.safe_exploration.run returned for the small sweep of
tests/test_estimator_batch_gpu.py (no guess_param) at the commit BEFORE the computed-simulator route was added -- run
there, on the GPU, from the repository root:  python tests/golden/make_safe_exploration_small.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from swimmer_amd.ars import safe_exploration  # noqa: E402

tmp = tempfile.mkdtemp()
out = safe_exploration.run(A_values=(0.5,), epsilons=[0.001], n_seed=2, n_iter=2, hand_iter=10, H=20,
                           rng=np.random.RandomState(7), results_path=os.path.join(tmp, "results"),
                           data_path=os.path.join(tmp, "data"))
np.savez(os.path.join(ROOT, "tests", "golden", "safe_exploration_small.npz"), r_graphs=out["r_graphs"],
         l=np.float64(out["l"]))
