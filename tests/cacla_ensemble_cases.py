"""The parity cases of the ensemble gate of CACLA on the swimmer, shared by tests/test_cacla_ensemble_cpu.py (which
asserts that they are sound) and tests/test_cacla_ensemble_gpu.py (which runs the kernel on them): the inputs of
tests/test_cacla_safe_gpu.py -- its six CASES with their thresholds, weights, noise, 96 steps, gamma and alpha -- with
the look-ahead in an ensemble on the epsilon-sphere around that file's simulator, and the oracle's run of each,
computed once."""
import numpy as np

import test_cacla_safe_gpu as single          # CASES, inputs(), costs(): the single-simulator cases, as they are
from swimmer_amd.ars import ensemble as ens
from swimmer_amd.ars.parameters import EnvParam

import cacla_ensemble_oracle as oracle_ens

CENTRE = single.SIM                           # (l_i, m_i, k) = (1.02, 0.97, 10.3); the real swimmer is (1, 1, 10)
SEED = 7
# tag: (the single-simulator case, members, epsilon).  The six cases in 5 members; then two wrap cases each at n = 3
# and n = 6 (one and two hidden units per lane): 7 members, which 64 lanes are no multiple of, and a full wave of 64
CASES = {tag: (tag, 5, 0.1) for tag in single.CASES}
CASES.update({"n3_e7": ("n3", 7, 0.2), "n6_e7": ("n6", 7, 0.2), "n3_e64": ("n3", 64, 0.1), "n6_e64": ("n6", 64, 0.1)})
_members, _oracle = {}, {}


def members(n, E, epsilon):
    """sphere_ensemble around the centre: member 0 is the centre itself.  -> (the EnvParams, rows [E, 3])"""
    key = (n, E, epsilon)
    if key not in _members:
        centre = EnvParam("centre", n, 0, CENTRE[0], CENTRE[1], 1e-3, CENTRE[2], 0.0)
        got = ens.sphere_ensemble(centre, epsilon, E, rng=np.random.RandomState(SEED))
        _members[key] = (got, ens.sim_rows(got))
    return _members[key]


def inputs(tag):
    """-> n, cost kind, weights, noise, sim_thresh, real_thresh, rows [E, 3]"""
    base, E, epsilon = CASES[tag]
    n, kind, w, noise, sim_thr, real_thr = single.inputs(base)
    return n, kind, w, noise, sim_thr, real_thr, members(n, E, epsilon)[1]


def want(tag):
    """The ensemble oracle's run of a case, computed once and left unchanged."""
    if tag not in _oracle:
        n, kind, w, noise, sim_thr, real_thr, rows = inputs(tag)
        _oracle[tag] = oracle_ens.run(n, single.GAMMA, single.ALPHA, w, noise, single.costs(kind)[1], rows, sim_thr,
                                      real_thr)
    return _oracle[tag]
