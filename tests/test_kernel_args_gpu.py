"""Every tensor-taking wrapper of swimmer_amd.kernels refuses every wrong tensor before the library is reached.

No kernel is launched: kernels.load is replaced by a stand-in that forwards the three host-only size helpers to the
real library and, for any other entry point, records the name and returns 0 WITHOUT calling it -- a check that misses
fails the test instead of writing out of bounds.  The GPU is needed for device tensors only.

CASES has one entry per wrapper with valid arguments at the smallest shapes (n = 3, 2 environments / rollouts, H = 2,
S = 2 agents, N = 1 direction, T = 3 transitions, 2 candidates, 2 sets, world = 2).  The valid call must reach the
stand-in exactly once.  Then every tensor parameter in turn is replaced by: another dtype; a tensor one short; a
non-contiguous view of the right shape; the same tensor on the CPU; the same tensor on cuda:1 where there is one.
Each must raise SwimmerHipError naming the parameter -- at the start of the message, or, for the tensor that sets
the call's device, as the "as NAME" behind the device another tensor is then refused for.

"One short" is the leading dimension less one.  Where that dimension is a lower bound the tensor is one below the
bound; where it DEFINES a size of the call (n_roll of `policies`, S of `policy`, ...) one fewer is another valid call,
so the first dimension that the call does fix is shortened instead; `send` of all_gather has no such dimension.  A
tensor with a single element is contiguous whatever its strides: it has no non-contiguous view to try.
"""
import inspect

import pytest
import torch

from test_kernel_args_cpu import SIGNATURES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, I32, I64, U8 = torch.float64, torch.int32, torch.int64, torch.uint8
OTHER = {F64: torch.float32, I32: I64, I64: I32, U8: I32}
D, M = 8, 2                                         # n = 3
HOST_ONLY = ("sw_moments_blocks", "sw_step_residual_blocks", "sw_cov_acc_doubles")
NO_TENSORS = {"ArsPipeline.__init__", "ArsPipeline.close", "ArsPipeline.host_slot_wait", "ArsPipeline.next_slot",
              "ArsPipeline.rollout_ms", "ArsPipeline.sync_cov", "ArsPipeline.timing", "DirectComm.__init__",
              "DirectComm.close", "SingleEnv.__init__", "SingleEnv.accelerations", "SingleEnv.close", "SingleEnv.step",
              "StepPlan.launch", "cacla_net_doubles", "cov_acc_doubles", "issue_interval_full_chip_ns",
              "issue_interval_ns", "lqr_model_doubles", "lqr_param_doubles", "moments_blocks", "new_cov_acc",
              "step_residual_blocks"}
UNCHECKED = {"ArsPipeline.rollouts", "ArsPipeline.update"}     # the documented exception: the agent's own buffers


@pytest.fixture(scope="module")
def sw():
    import swimmer_amd
    swimmer_amd._lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return swimmer_amd


class StandIn(object):
    """In place of the loaded library: the host-only size helpers are the real ones, anything else is recorded and
    not called."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in HOST_ONLY:
            return getattr(self.real, name)

        def record(*args):
            self.calls.append(name)
            return 0
        return record


@pytest.fixture
def lib(sw, monkeypatch):
    stand_in = StandIn(sw._lib.load())
    monkeypatch.setattr(sw.kernels, "load", lambda: stand_in)
    return stand_in


class T(object):
    """A tensor argument: dtype, the valid shape, and the shape that is one short (default: leading dimension - 1;
    None: there is none)."""

    def __init__(self, dtype, *shape, short="leading"):
        self.dtype, self.shape = dtype, shape
        self.short = (shape[0] - 1,) + shape[1:] if short == "leading" else short

    def make(self, device=DEV):
        return torch.zeros(self.shape, dtype=self.dtype, device=device)


def f(*shape, **kw):
    return T(F64, *shape, **kw)


def i(*shape, **kw):
    return T(I32, *shape, **kw)


def _plan(sw):
    def call(**kw):
        sw.kernels.StepPlan(**kw).launch()
    return call


def _all_gather(sw):
    def call(**kw):
        comm = object.__new__(sw.kernels.DirectComm)        # the constructor is a collective over RCCL
        comm._h, comm._lib, comm.world, comm.rank = None, sw.kernels.load(), 2, 0
        comm._fn = comm._lib.sw_comm_all_gather_f64
        comm.all_gather(**kw)
    return call


def cases(sw):
    """{wrapper: (callable, scalar arguments, {parameter: T})}."""
    k = sw.kernels
    p = sw.SwParams.make(3)
    nb3, nb2, mb = k.step_residual_blocks(3), k.step_residual_blocks(2), k.moments_blocks(2)
    acc = k.cov_acc_doubles(p, 2, 2)
    transitions = dict(state=f(D, 3), action=f(M, 3), next_ref=f(D, 3))
    envs = dict(state=f(D, 2), action=f(M, 2))
    pair, pair_s = dict(mean=f(D), inv_std=f(D)), dict(mean=f(2, D), inv_std=f(2, D))
    multi = dict(policy=f(2, M, D, short=(2, M - 1, D)), deltas=f(2, 1, M, D))
    sets = dict(set_begin=T(I64, 3, short=(1,)), **transitions)                    # the bound: two entries, one set
    upd = dict(policy=f(M, D), running=f(1 + 2 * D), sigma_out=f(1), **pair)
    upd_s = dict(returns=f(2, 2, short=(2, 1)), deltas=f(2, 1, M, D), policy=f(2, M, D), running=f(2, 1 + 2 * D),
                 sigma_out=f(2), **pair_s)
    ints = dict(first_refused=i(2), violations=i(2), status=i(2))
    return {
        "reset": (k.reset, dict(p=p, n_env=2, device=DEV), dict(out=f(D, 2))),
        "step": (k.step, dict(p=p), dict(out=f(D, 2), reward=f(2), status=i(2), **envs)),
        "StepPlan.__init__": (_plan(sw), dict(p=p), dict(out=f(D, 2), reward=f(2), status=i(2), **envs)),
        "accelerations": (k.accelerations, dict(p=p), envs),
        "step_residual": (k.step_residual, dict(p=p), dict(partial=f(nb3), **transitions)),
        "step_residual_population": (k.step_residual_population, dict(p_base=p), dict(
            cand=f(2, 3, short=(2, 2)), partial=f(2, nb3), value=f(2), status=i(2), **transitions)),
        "step_residual_sets": (k.step_residual_sets, dict(p_base=p, max_set_len=2), dict(
            cand=f(2, 3, short=(2, 2)), cand_set=i(2), partial=f(2, nb2), value=f(2), status=i(2), **sets)),
        "step_residual_normal_sets": (k.step_residual_normal_sets, dict(p_base=p, max_set_len=2), dict(
            points=f(2, 7, 3), inv_2e=f(2, 3), active=i(2), partial=f(2, 13, nb2), out=f(2, 13), status=i(2), **sets)),
        "DirectComm.all_gather": (_all_gather(sw), {}, dict(send=f(4, short=None), gathered=f(8))),
        "rollout": (k.rollout, dict(p=p, H=2), dict(
            policies=f(2, M, D, short=(2, M - 1, D)), state0=f(D, 2), traj=f(2, D, 2), final_state=f(D, 2),
            moments=f(mb, 2 * D), status=i(2), returns=f(2), **pair)),
        "safe_rollouts": (k.safe_rollouts, dict(p_real=p, p_sim=p, H=2, cost_kind=0, cost_index=3, sim_thresh=1.0,
                                                real_thresh=1.0), dict(
            policies=f(2, M, D, short=(2, M - 1, D)), traj=f(2, D, 2), returns=f(2), **ints)),
        "ars_rollouts": (k.ars_rollouts, dict(p=p, H=2, nu=0.01, dir_begin=1, n_dir=1), dict(
            policy=f(M, D), deltas=f(2, M, D), returns=f(2), traj=f(2, D, 2), moments=f(mb, 2 * D), status=i(2),
            **pair)),
        "ars_gate": (k.ars_gate, dict(p_sim=p, H=2, nu=0.01, dir_begin=1, n_dir=1, sim_thresh=0.0), dict(
            policy=f(M, D), deltas=f(2, M, D), returns=f(2), status=i(2), admit=i(1), **pair)),
        "ars_update": (k.ars_update, dict(p=p, alpha=0.01, b=1.0, top_b=1, n_new_states=4), dict(
            returns=f(2), deltas=f(1, M, D), moments=f(1, 2 * D, short=(1, 2 * D - 1)), **upd)),   # any row count
        "ars_update_gathered": (k.ars_update_gathered, dict(p=p, n_dir=1, world=2, chunk=1, rows_chunk=1, alpha=0.01,
                                                            b=1.0, top_b=1, n_new_states=4), dict(
            gathered=f(2 * (2 + 2 * D)), deltas=f(1, M, D), **upd)),
        "ars_rollouts_multi": (k.ars_rollouts_multi, dict(p=p, H=2, nu=0.01), dict(
            returns=f(2, 2), moments=f(2, mb, 2 * D), status=i(2, 2), **multi, **pair_s)),
        "ars_rollouts_multi_counted": (k.ars_rollouts_multi_counted, dict(p=p, H=2, nu=0.01), dict(
            count=i(2), returns=f(2, 2), moments=f(2, mb, 2 * D), status=i(2, 2), **multi, **pair_s)),
        "ars_gate_multi": (k.ars_gate_multi, dict(p_base=p, H=2, nu=0.01), dict(
            sim=f(2, 3), sim_thresh=f(2), returns=f(2, 2), status=i(2, 2), admit=i(2, 1), **multi, **pair_s)),
        "ars_pack_admitted": (k.ars_pack_admitted, dict(p=p), dict(
            admit=i(2, 1, short=(2, 0)), deltas=f(2, 1, M, D), status=i(2, 2), count=i(2), order=i(2, 1),
            packed=f(2, 1, M, D))),
        "ars_update_multi": (k.ars_update_multi, dict(p=p, alpha=0.01, b=1.0, top_b=1, n_new_states=4), dict(
            moments=f(2, 1, 2 * D), **upd_s)),
        "ars_update_multi_counted": (k.ars_update_multi_counted, dict(p=p, H=2, alpha=0.01, b=1.0, top_b=1), dict(
            count=i(2), moments=f(2, mb, 2 * D, short=(2, mb - 1, 2 * D)), **upd_s)),      # one below the bound
        "safe_ars_rollouts_multi": (k.safe_ars_rollouts_multi, dict(p_real=p, H=2, nu=0.01, cost_kind=0, cost_index=3),
                                    dict(gated=i(2), sim=f(2, 3), sim_thresh=f(2), real_thresh=f(2), returns=f(2, 2),
                                         cost_trace=f(2, 2, 2), cost_max=f(2, 2), first_refused=i(2, 2),
                                         violations=i(2, 2), status=i(2, 2), **multi)),
        "cacla_run": (k.cacla_run, dict(p=p, n_iter=2, train=True), dict(
            gamma=f(2, short=(0,)), alpha=f(2), noise=f(2, 2, M), weights=f(2, 3, k.cacla_net_doubles(3)),
            state=f(2, D), rewards=f(2, 2), actor_updates=i(2), status=i(2))),
        "traj_moments": (k.traj_moments, dict(p=p), dict(traj=f(2, D, 2, short=(2, D - 1, 2)), acc=f(acc))),
        "lqr_cacla_run": (k.lqr_cacla_run, dict(ns=2, na=1, n_iter=2, safe=True, threshold=0, cost=0), dict(
            params=f(k.lqr_param_doubles(2, 1), 2), noise=f(2, 1, 2), F=f(1, 2, 2), V=f(2, 2), state=f(2, 2),
            last=f(4, 2), counters=i(3, 2), status=i(2), rec_state=f(2, 2, 2), rec_action=f(2, 1, 2),
            rec_reward=f(2, 2), rec_admitted=T(U8, 2, 2))),
    }


NAMES = sorted(set(SIGNATURES) - NO_TENSORS - UNCHECKED)


def test_the_table_has_every_wrapper_that_takes_a_tensor(sw, lib):
    table = cases(sw)
    assert sorted(table) == NAMES
    for name, (_, scalars, tensors) in table.items():            # and every parameter of each
        obj = sw.kernels
        for part in name.split("."):
            obj = getattr(obj, part)
        params = [q for q in inspect.signature(obj).parameters if q != "self"]
        assert sorted(params) == sorted(list(scalars) + list(tensors)), name
    assert not lib.calls


@pytest.mark.parametrize("name", NAMES)
def test_every_wrong_tensor_is_refused_by_name_before_the_library(sw, lib, name):
    call, scalars, tensors = cases(sw)[name]
    valid = dict(scalars, **{q: t.make() for q, t in tensors.items()})
    call(**valid)
    assert len(lib.calls) == 1, lib.calls                         # without this the mutations below prove nothing
    del lib.calls[:]
    tried = 0
    for q, t in tensors.items():
        wrong = {"dtype": torch.zeros(t.shape, dtype=OTHER[t.dtype], device=DEV),
                 "view": torch.zeros(t.shape + (2,), dtype=t.dtype, device=DEV)[..., 0],
                 "cpu": valid[q].cpu()}
        if t.short is not None:
            wrong["short"] = torch.zeros(t.short, dtype=t.dtype, device=DEV)
        if torch.cuda.device_count() >= 2:
            wrong["cuda:1"] = valid[q].to("cuda:1")
        assert tuple(wrong["view"].shape) == t.shape
        if wrong["view"].is_contiguous():
            assert wrong["view"].numel() == 1
            del wrong["view"]
        for what, bad in wrong.items():
            with pytest.raises(sw.SwimmerHipError, match=rf"^{q}: expected | as {q}, got ") as e:
                call(**dict(valid, **{q: bad}))
            assert not lib.calls, (q, what, "reached", lib.calls)
            assert what == "cuda:1" or str(e.value).startswith(q + ": "), (q, what, str(e.value))
            tried += 1
    assert tried >= 3 * len(tensors)


@pytest.mark.parametrize("name", NAMES)
def test_optional_tensors_may_be_left_out(sw, lib, name):
    """Every parameter with the default None left out together: the call still reaches the library once."""
    call, scalars, tensors = cases(sw)[name]
    obj = sw.kernels
    for part in name.split("."):
        obj = getattr(obj, part)
    required = {q for q, par in inspect.signature(obj).parameters.items() if par.default is inspect.Parameter.empty}
    call(**dict(scalars, **{q: t.make() for q, t in tensors.items() if q in required}))
    assert len(lib.calls) == 1, lib.calls


def test_running_needs_its_moments(sw, lib):
    for wrapper in ("ars_update", "ars_update_multi", "ars_update_multi_counted"):
        call, scalars, tensors = cases(sw)[wrapper]
        kw = dict(scalars, **{q: t.make() for q, t in tensors.items() if q != "moments"})
        with pytest.raises(sw.SwimmerHipError, match=r"^moments: expected .* got None"):
            call(**kw)
        assert not lib.calls, wrapper


def test_mean_and_inv_std_are_given_together(sw, lib):
    with_pair = [name for name in NAMES if {"mean", "inv_std"} <= set(cases(sw)[name][2])]
    assert with_pair == ["ars_gate", "ars_gate_multi", "ars_rollouts", "ars_rollouts_multi",
                         "ars_rollouts_multi_counted", "ars_update", "ars_update_gathered", "ars_update_multi",
                         "ars_update_multi_counted", "rollout"]
    for name in with_pair:
        call, scalars, tensors = cases(sw)[name]
        for given, missing in (("mean", "inv_std"), ("inv_std", "mean")):
            # without running (and its moments): next to running both are required anyway
            kw = dict(scalars, **{q: t.make() for q, t in tensors.items() if q not in (missing, "running", "moments")})
            with pytest.raises(sw.SwimmerHipError, match=rf"^{missing}: expected .* got None"):
                call(**kw)
            assert not lib.calls, (name, given)
