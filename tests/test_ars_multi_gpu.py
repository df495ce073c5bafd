"""sw_ars_rollouts_multi_f64 / sw_ars_update_multi_f64 against their single-agent entry points, agent by agent and
bit for bit.  Every agent has its own policy, deltas and (V2) statistics, so a kernel that reads another agent's
data, mixes agents in a moment row or lets a padding slot count cannot pass."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:      # the quad-form child below runs this file as a script
    sys.path.insert(0, ROOT)

import swimmer_amd as sw  # noqa: E402
from swimmer_amd import kernels  # noqa: E402

from batch_kernel_cases import (MORE_INSTANTIATIONS, MORE_S, MULTI_AGENTS, MULTI_DIRS, MULTI_FORMS,  # noqa: E402
                                MULTI_NS, more_id)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = 60
NU = 0.05


def _agent_inputs(n, N, S, v2, seed=0):
    """Per agent: a random policy in (-1, 1), its own deltas and, for V2, its own mean in (-0.1, 0.1) and inv_std in
    (0.5, 2) -- the ranges of _gate_inputs in tests/test_safe_ars_agent_gpu.py."""
    m, d = n - 1, 2 * n + 2
    rng = np.random.RandomState(100000 * seed + 1000 * n + 10 * N + S)
    policy = torch.tensor(rng.uniform(-1, 1, (S, m, d)), device=DEV)
    deltas = torch.tensor(2 * rng.rand(S, N, m, d) - 1, device=DEV)
    mean = inv_std = None
    if v2:
        mean = torch.tensor(rng.uniform(-0.1, 0.1, (S, d)), device=DEV)
        inv_std = torch.tensor(rng.uniform(0.5, 2.0, (S, d)), device=DEV)
    return policy, deltas, mean, inv_std


def _compare_rollouts(p, n, N, S, v2, with_moments=True):
    """Multi launch (outputs poisoned first) against one ars_rollouts call per agent; returns the number of agents.
    with_moments False: neither side is given a moments buffer -- the segment-per-lane forms then run their MOM = false
    kernels -- and returns and status are what is compared."""
    policy, deltas, mean, inv_std = _agent_inputs(n, N, S, v2)
    rows = kernels.moments_blocks(2 * N)
    returns = torch.full((S, 2 * N), float("nan"), dtype=torch.float64, device=DEV)
    moments = torch.full((S, rows, 2 * p.d), float("nan"), dtype=torch.float64, device=DEV) if with_moments else None
    status = torch.full((S, 2 * N), -1, dtype=torch.int32, device=DEV)
    out = kernels.ars_rollouts_multi(p, H, policy, deltas, NU, mean, inv_std, returns=returns, moments=moments,
                                     status=status)
    assert out is returns
    R, St = returns.cpu().numpy(), status.cpu().numpy()
    M = moments.cpu().numpy() if with_moments else None
    assert not np.isnan(R).any() and (M is None or not np.isnan(M).any()), "an output cell was left unwritten"
    assert (St == 0).all()
    for a in range(S):
        mom1 = torch.zeros((rows, 2 * p.d), dtype=torch.float64, device=DEV) if with_moments else None
        st1 = torch.full((2 * N,), -1, dtype=torch.int32, device=DEV)
        r1 = kernels.ars_rollouts(p, H, policy[a], deltas[a], NU, 0, N, None if mean is None else mean[a],
                                  None if inv_std is None else inv_std[a], moments=mom1, status=st1)
        assert (st1.cpu().numpy() == 0).all()
        assert np.array_equal(R[a], r1.cpu().numpy()), (a, "returns")
        if with_moments:
            assert np.array_equal(M[a], mom1.cpu().numpy()), (a, "moment rows")
    return S


@pytest.mark.parametrize("v2", [False, True], ids=["V1", "V2"])
@pytest.mark.parametrize("form", MULTI_FORMS)
@pytest.mark.parametrize("S", MULTI_AGENTS)
@pytest.mark.parametrize("N", MULTI_DIRS)        # 2N = 2, 14, 16, 18: below, just below, exactly, across a moment row
@pytest.mark.parametrize("n", MULTI_NS)          # lane only, mirror-quad, row
def test_multi_rollouts_equal_single_agent_launches(n, N, S, form, v2):
    # auto: S * 16 * ceil(2N / 16) <= 288 slots, far below 8192 -- the batch and the single launches take the same form
    p = sw.SwParams.make(n, 0.8, 1.2, 10.2, 1e-3, flags=sw._lib.kernel_flags(form))
    _compare_rollouts(p, n, N, S, v2)


# Every compiled instantiation that the product above does not reach (it always asks for moments, so its segment-per-lane
# launches are all MOM = true), S = 3 agents each: (form, twin model, n, N, V2, moments asked for).
#  * ars_multi_row_kernel<N, MOM>, N = 4, 5, 7, 8 (each with a loop pad of its own per MOM): a V1 agent asks for no
#    moments, MOM = false; a V2 agent does, MOM = true; 2N = 14 and 18: just below and across a moment row.  N = 6 with
#    MOM = false too, which the product leaves out.  MOM follows the moments pointer alone: one V2 launch without
#    moments (whitening, MOM = false) at n = 5.
#  * ars_multi_lane_kernel<N, false> at the same n.
#  * ars_multi_lane_kernel<N, true>, every n = 2..8: the twin model (its single-agent rollouts are held to the twin
#    oracle at every n in tests/test_rollout_matrix_gpu.py, the twin cases; equality with them is the reference here).
# The n = 3 forms without moments: test_multi_rollouts_without_moments_and_status (mirror-quad) and the quad child.
# The list itself is MORE_INSTANTIATIONS of tests/batch_kernel_cases.py, where tests/test_batch_kernels_cpu.py derives
# from it which kernels are launched.
@pytest.mark.parametrize("form,twin,n,N,v2,with_moments", MORE_INSTANTIATIONS,
                         ids=[more_id(*case) for case in MORE_INSTANTIATIONS])
def test_multi_rollouts_at_every_compiled_n_and_model(form, twin, n, N, v2, with_moments):
    flags = sw._lib.kernel_flags(form) | (sw._lib.FLAG_MODEL_TWIN if twin else 0)
    p = sw.SwParams.make(n, 0.8, 1.2, 10.2, 1e-3, flags=flags)
    _compare_rollouts(p, n, N, MORE_S, v2, with_moments)


def test_multi_rollouts_without_moments_and_status():
    """The optional outputs left out: V1 agents as ARSAgentBatch launches them."""
    p = sw.SwParams.make(3)
    policy, deltas, _, _ = _agent_inputs(3, 9, 3, False)
    R = kernels.ars_rollouts_multi(p, H, policy, deltas, NU).cpu().numpy()
    for a in range(3):
        assert np.array_equal(R[a], kernels.ars_rollouts(p, H, policy[a], deltas[a], NU, 0, 9).cpu().numpy())


def test_quad3_multi_form_in_a_child_process():
    """SWIMMER_N3_KERNEL=quad (read once per process) sends n = 3 to the quad form: batch and single launches alike."""
    env = dict(os.environ, SWIMMER_N3_KERNEL="quad")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "quad-child"], env=env, capture_output=True,
                          text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "quad-child ok" in done.stdout


def _update_inputs(rng, S, N, d, m, rows, count):
    returns = torch.tensor(rng.uniform(-3, 3, (S, 2 * N)), device=DEV)
    deltas = torch.tensor(2 * rng.rand(S, N, m, d) - 1, device=DEV)
    x = rng.normal(0.0, 1.0, (S, rows, count, d)) * rng.uniform(0.5, 2.0, (S, 1, 1, d))
    moments = torch.tensor(np.concatenate([x.sum(axis=2), (x * x).sum(axis=2)], axis=2), device=DEV)
    return returns, deltas, moments


@pytest.mark.parametrize("v2", [False, True], ids=["V1", "V2"])
@pytest.mark.parametrize("top_b", [0, 4])
@pytest.mark.parametrize("N", [1, 9, 300])
def test_multi_update_equals_single_agent_updates(N, top_b, v2):
    _compare_updates(N, top_b, v2)


def test_multi_update_with_wide_workgroups():
    """N = 1025 directions: the first count at which the update kernels run 1024-thread workgroups (kUpdWideFrom)."""
    _compare_updates(1025, 4, True)


def _compare_updates(N, top_b, v2):
    n, S, count = 3, 3, 40
    p = sw.SwParams.make(n)
    m, d = p.m, p.d
    rows = kernels.moments_blocks(2 * N)
    rng = np.random.RandomState(7 * N + top_b)
    f64 = dict(dtype=torch.float64, device=DEV)
    policy = torch.tensor(rng.uniform(-1, 1, (S, m, d)), device=DEV)
    running = torch.zeros((S, 1 + 2 * d), **f64) if v2 else None
    mean = torch.zeros((S, d), **f64) if v2 else None
    inv_std = torch.ones((S, d), **f64) if v2 else None
    sigma = torch.zeros(S, **f64)
    # the single-agent state, agent by agent
    one = [dict(policy=policy[a].clone(), running=None if not v2 else running[a].clone(),
                mean=None if not v2 else mean[a].clone(), inv_std=None if not v2 else inv_std[a].clone(),
                sigma=torch.zeros(1, **f64)) for a in range(S)]
    n_new = rows * count
    for call in range(2):       # the second call merges into running statistics that are no longer zero
        returns, deltas, moments = _update_inputs(rng, S, N, d, m, rows, count)
        kernels.ars_update_multi(p, returns, deltas, policy, 0.02, float(N), top_b, moments=moments if v2 else None,
                                 running=running, n_new_states=n_new, mean=mean, inv_std=inv_std, sigma_out=sigma)
        for a, o in enumerate(one):
            kernels.ars_update(p, returns[a], deltas[a], o["policy"], 0.02, float(N), top_b,
                               moments=moments[a] if v2 else None, running=o["running"], n_new_states=n_new,
                               mean=o["mean"], inv_std=o["inv_std"], sigma_out=o["sigma"])
            assert np.array_equal(policy[a].cpu().numpy(), o["policy"].cpu().numpy()), (call, a, "policy")
            assert np.array_equal(sigma[a:a + 1].cpu().numpy(), o["sigma"].cpu().numpy()), (call, a, "sigma")
            if v2:
                for name, t in (("running", running), ("mean", mean), ("inv_std", inv_std)):
                    assert np.array_equal(t[a].cpu().numpy(), o[name].cpu().numpy()), (call, a, name)
    assert np.isfinite(policy.cpu().numpy()).all()
    if v2:
        assert (running[:, 0].cpu().numpy() == 2 * n_new).all()


def test_argument_errors_leave_the_outputs_alone():
    p = sw.SwParams.make(3)
    S, N = 2, 3
    policy, deltas, mean, inv_std = _agent_inputs(3, N, S, True)
    returns = torch.full((S, 2 * N), 7.0, dtype=torch.float64, device=DEV)
    status = torch.full((S, 2 * N), -1, dtype=torch.int32, device=DEV)
    lib, ptr, ok = sw._lib.load(), sw._lib.ptr, ctypes.byref(p)

    def roll(S_=S, N_=N, pol=policy, dl=deltas, mn=mean, isd=inv_std, ret=returns, params=ok):
        return lib.sw_ars_rollouts_multi_f64(params, S_, N_, H, ptr(pol), ptr(dl), NU, ptr(mn), ptr(isd), ptr(ret),
                                             None, ptr(status), None)
    assert roll(S_=0) == 3                     # SW_ERR_SIZE
    assert roll(N_=0) == 3
    assert roll(pol=None) == 1                 # SW_ERR_NULL
    assert roll(dl=None) == 1
    assert roll(ret=None) == 1
    assert roll(isd=None) == 1                 # mean without inv_std
    assert roll(mn=None) == 1
    assert roll(params=None) == 1
    assert roll(params=ctypes.byref(sw.SwParams.make(9))) == 2
    upd = lib.sw_ars_update_multi_f64
    before = policy.clone()
    assert upd(ok, 0, N, ptr(returns), ptr(deltas), ptr(policy), 0.01, 1.0, 0, None, 0, None, 0, None, None, None,
               None) == 3
    assert upd(ok, S, 0, ptr(returns), ptr(deltas), ptr(policy), 0.01, 1.0, 0, None, 0, None, 0, None, None, None,
               None) == 3
    assert upd(ok, S, N, None, ptr(deltas), ptr(policy), 0.01, 1.0, 0, None, 0, None, 0, None, None, None,
               None) == 1
    torch.cuda.synchronize()
    assert (returns.cpu().numpy() == 7.0).all() and (status.cpu().numpy() == -1).all()
    assert np.array_equal(policy.cpu().numpy(), before.cpu().numpy())
    with pytest.raises(sw.SwimmerHipError):
        kernels.ars_rollouts_multi(p, H, policy, deltas, NU, mean, None)
    with pytest.raises(sw.SwimmerHipError):
        kernels.ars_rollouts_multi(p, H, policy, deltas[:1], NU)
    with pytest.raises(sw.SwimmerHipError):
        kernels.ars_update_multi(p, returns, deltas[:, :2], policy, 0.01, 1.0)


if __name__ == "__main__" and sys.argv[1:] == ["quad-child"]:
    # the child of test_quad3_multi_form_in_a_child_process: 2N = 18 crosses a moment row, V1 and V2; and V1 without
    # moments: ars_multi_quad3_kernel<false>
    for v2_ in (False, True):
        _compare_rollouts(sw.SwParams.make(3, 0.8, 1.2, 10.2, 1e-3), 3, 9, 3, v2_)
    _compare_rollouts(sw.SwParams.make(3, 0.8, 1.2, 10.2, 1e-3), 3, 9, 3, False, with_moments=False)
    print("quad-child ok")
