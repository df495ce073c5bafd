"""The one tensor-argument check of swimmer_amd.kernels (_tensor, with its forms _opt and _out) on CPU tensors, and
the frozen public interface of the module.  tests/test_kernel_args_gpu.py drives every wrapper through the check."""
import inspect

import pytest
import torch

import swimmer_amd as sw
from swimmer_amd import kernels as k

CPU = (torch.device("cpu"), "x")
SHAPE = (8, 4)


def _good(dtype=torch.float64):
    return torch.zeros(SHAPE, dtype=dtype)


def test_a_right_tensor_passes_through_as_the_same_object():
    t = _good()
    assert k._tensor(t, "x", SHAPE, CPU) is t
    assert k._opt(t, "x", SHAPE, CPU) is t
    assert k._out(t, "x", SHAPE, CPU) is t
    i = _good(torch.int32)
    assert k._tensor(i, "x", SHAPE, CPU, torch.int32) is i
    assert k._opt(None, "x", SHAPE, CPU) is None


def test_a_lower_bound_entry_takes_the_bound_and_more_but_not_less():
    t = _good()
    for shape in ((k._Min(8), 4), (k._Min(7), 4), (k._ANY, 4), (8, k._Min(0))):
        assert k._tensor(t, "x", shape, CPU) is t
    for shape in ((k._Min(9), 4), (k._Min(7), 5), (k._Min(8),), (k._Min(8), 4, k._ANY)):
        with pytest.raises(sw.SwimmerHipError, match=r"^x: .*>="):
            k._tensor(t, "x", shape, CPU)


BAD = {
    "wrong dtype": lambda: _good(torch.float32),
    "other integer dtype": lambda: _good(torch.int64),
    "one row short": lambda: torch.zeros((7, 4), dtype=torch.float64),
    "one dimension more": lambda: torch.zeros((8, 4, 1), dtype=torch.float64),
    "flat": lambda: torch.zeros(32, dtype=torch.float64),
    "non-contiguous view of the right shape": lambda: torch.zeros(SHAPE + (2,), dtype=torch.float64)[..., 0],
    "transposed": lambda: torch.zeros((4, 8), dtype=torch.float64).t(),
    "other device": lambda: torch.zeros(SHAPE, dtype=torch.float64, device="meta"),
    "not a tensor": lambda: [[0.0] * 4] * 8,
}


@pytest.mark.parametrize("what", sorted(BAD))
@pytest.mark.parametrize("form", ("_tensor", "_opt", "_out"))
def test_every_miss_is_a_SwimmerHipError_that_names_the_parameter(form, what):
    t = BAD[what]()
    if "right shape" in what or what in ("transposed", "other device"):
        assert tuple(t.shape) == SHAPE
    with pytest.raises(sw.SwimmerHipError, match=r"^some_name: expected a contiguous torch.float64 tensor of shape "
                                                 r"\(8, 4\) on cpu as x, got ") as e:
        getattr(k, form)(t, "some_name", SHAPE, CPU)
    given = {"wrong dtype": "float32", "other integer dtype": "int64", "one row short": "(7, 4)",
             "one dimension more": "(8, 4, 1)", "flat": "(32,)", "non-contiguous view of the right shape":
             "not contiguous", "transposed": "not contiguous", "other device": "meta", "not a tensor": "list"}[what]
    assert given in str(e.value)


def test_none_is_refused_where_the_tensor_is_required():
    with pytest.raises(sw.SwimmerHipError, match=r"^x: .*got None"):
        k._tensor(None, "x", SHAPE, CPU)


def test_mean_and_inv_std_come_together():
    m = torch.zeros(8, dtype=torch.float64)
    k._pair(None, None, (8,), CPU)
    k._pair(m, m.clone(), (8,), CPU)
    with pytest.raises(sw.SwimmerHipError, match=r"^inv_std: "):
        k._pair(m, None, (8,), CPU)
    with pytest.raises(sw.SwimmerHipError, match=r"^mean: "):
        k._pair(None, m, (8,), CPU)
    with pytest.raises(sw.SwimmerHipError, match=r"^mean: "):
        k._pair(None, None, (8,), CPU, required=True)


def test_the_first_required_tensor_must_be_on_a_gpu():
    with pytest.raises(sw.SwimmerHipError, match=r"^state: expected a 2-D tensor on the GPU, got torch.float64 \(8, 4\)"):
        k._gpu(_good(), "state", 2)
    with pytest.raises(sw.SwimmerHipError, match=r"^state: .*got int"):
        k._gpu(3, "state", 2)


def test_the_output_form_allocates_what_it_is_asked_for():
    e = k._out(None, "x", SHAPE, CPU)
    assert e.dtype == torch.float64 and tuple(e.shape) == SHAPE and e.device.type == "cpu" and e.is_contiguous()
    z = k._out(None, "x", (3,), CPU, torch.int32, fill=0)
    assert z.dtype == torch.int32 and tuple(z.shape) == (3,) and not z.any()
    z = k._out(None, "x", SHAPE, CPU, fill=0.0)
    assert z.dtype == torch.float64 and tuple(z.shape) == SHAPE and not z.any()
    nan = k._out(None, "x", (2, 5), CPU, fill=float("nan"))
    assert nan.dtype == torch.float64 and tuple(nan.shape) == (2, 5) and bool(torch.isnan(nan).all())
    acc = k._out(None, "x", (k._Min(6),), CPU, fill=0.0)           # a bound allocates the bound
    assert tuple(acc.shape) == (6,) and not acc.any()
    assert k._out(None, "x", SHAPE, (torch.device("meta"), "device")).device.type == "meta"


def test_without_a_gpu_every_wrapper_still_says_that_there_is_no_cpu_fallback():
    if torch.cuda.is_available():
        return
    p = sw.SwParams.make(3)
    t = torch.zeros((8, 2), dtype=torch.float64)
    for call in (lambda: k.reset(p, 2), lambda: k.step(p, t, t), lambda: k.step(p, None, None),
                 lambda: k.ars_update(p, None, None, None, 0.1, 1.0), lambda: k.traj_moments(p, 7),
                 lambda: k.StepPlan(p, t, t, t)):
        with pytest.raises(sw.SwimmerHipError, match="no CPU fallback"):
            call()


# Written from the parent commit, before kernels.py was touched: every public function, every public class's
# __init__ and public methods, with str(inspect.signature(...)).
P = "swimmer_amd._lib.SwParams"
SIGNATURES = {
    "ArsPipeline.__init__": "(self)",
    "ArsPipeline.close": "(self)",
    "ArsPipeline.host_slot_wait": "(self, slot)",
    "ArsPipeline.next_slot": "(self)",
    "ArsPipeline.rollout_ms": "(self)",
    "ArsPipeline.rollouts": "(self, slot, p, n_dir_total, dir_begin, n_dir, H, deltas_host, deltas_dev, policy, nu, "
                            "mean, inv_std, returns, traj, moments, cov_acc, status)",
    "ArsPipeline.sync_cov": "(self)",
    "ArsPipeline.timing": "(self, every)",
    "ArsPipeline.update": "(self, slot, p, n_dir, gathered, world, chunk, rows_chunk, deltas_dev, policy, alpha, b, "
                          "top_b, running, n_new_states, mean, inv_std, sigma_out)",
    "DirectComm.__init__": "(self, world, rank, broadcast_id, agree=None)",
    "DirectComm.all_gather": "(self, send, gathered)",
    "DirectComm.close": "(self)",
    "SingleEnv.__init__": "(self)",
    "SingleEnv.accelerations": f"(self, p: {P})",
    "SingleEnv.close": "(self)",
    "SingleEnv.step": f"(self, p: {P})",
    "StepPlan.__init__": f"(self, p: {P}, state, action, out, reward=None, status=None)",
    "StepPlan.launch": "(self)",
    "accelerations": f"(p: {P}, state, action)",
    "ars_gate": f"(p_sim: {P}, H: int, policy, deltas, nu: float, dir_begin: int, n_dir: int, sim_thresh: float, "
                "mean=None, inv_std=None, returns=None, status=None, admit=None)",
    "ars_gate_multi": f"(p_base: {P}, H: int, policy, deltas, nu: float, sim, sim_thresh, mean=None, inv_std=None, "
                      "returns=None, status=None, admit=None)",
    "ars_pack_admitted": f"(p: {P}, admit, deltas, status=None, count=None, order=None, packed=None)",
    "ars_rollouts": f"(p: {P}, H: int, policy, deltas, nu: float, dir_begin: int, n_dir: int, mean=None, "
                    "inv_std=None, returns=None, traj=None, moments=None, status=None)",
    "ars_rollouts_multi": f"(p: {P}, H: int, policy, deltas, nu: float, mean=None, inv_std=None, returns=None, "
                          "moments=None, status=None)",
    "ars_rollouts_multi_counted": f"(p: {P}, H: int, policy, deltas, nu: float, count, mean=None, inv_std=None, "
                                  "returns=None, moments=None, status=None)",
    "ars_update": f"(p: {P}, returns, deltas, policy, alpha: float, b: float, top_b: int = 0, moments=None, "
                  "running=None, n_new_states: int = 0, mean=None, inv_std=None, sigma_out=None)",
    "ars_update_gathered": f"(p: {P}, n_dir: int, gathered, world: int, chunk: int, rows_chunk: int, deltas, policy, "
                           "alpha: float, b: float, top_b: int = 0, running=None, n_new_states: int = 0, mean=None, "
                           "inv_std=None, sigma_out=None)",
    "ars_update_multi": f"(p: {P}, returns, deltas, policy, alpha: float, b: float, top_b: int = 0, moments=None, "
                        "running=None, n_new_states: int = 0, mean=None, inv_std=None, sigma_out=None)",
    "ars_update_multi_counted": f"(p: {P}, H: int, count, returns, deltas, policy, alpha: float, b: float, "
                                "top_b: int = 0, moments=None, running=None, mean=None, inv_std=None, sigma_out=None)",
    "cacla_net_doubles": "(n: int) -> int",
    "cacla_run": f"(p: {P}, n_iter: int, train: bool, gamma, alpha, noise, weights, state, rewards=None, "
                 "actor_updates=None, status=None)",
    "cov_acc_doubles": f"(p: {P}, n_roll: int, H: int) -> int",
    "issue_interval_full_chip_ns": "(mode: int, device='cuda:0', trips: int = 8192, workgroups: int = 256, "
                                   "waves: int = 4, settle_ms: float = 60.0)",
    "issue_interval_ns": "(mode: int, device='cuda:0', trips: int = 8192)",
    "lqr_cacla_run": "(ns: int, na: int, n_iter: int, safe: bool, threshold: int, cost: int, params, noise, F, V, "
                     "state, last, counters, status, rec_state=None, rec_action=None, rec_reward=None, "
                     "rec_admitted=None)",
    "lqr_model_doubles": "(ns: int, na: int) -> int",
    "lqr_param_doubles": "(ns: int, na: int) -> int",
    "moments_blocks": "(n_roll: int) -> int",
    "new_cov_acc": f"(p: {P}, n_roll: int, H: int, device)",
    "reset": f"(p: {P}, n_env: int, device='cuda:0', out=None)",
    "rollout": f"(p: {P}, H: int, policies, mean=None, inv_std=None, state0=None, traj=None, final_state=None, "
               "moments=None, status=None, returns=None)",
    "safe_ars_rollouts_multi": f"(p_real: {P}, H: int, policy, deltas, nu: float, gated, sim, sim_thresh, real_thresh, "
                               "cost_kind: int, cost_index: int, returns=None, cost_trace=None, cost_max=None, "
                               "first_refused=None, violations=None, status=None)",
    "safe_rollouts": f"(p_real: {P}, p_sim: {P}, H: int, policies, cost_kind: int, cost_index: int, "
                     "sim_thresh: float, real_thresh: float, traj=None, first_refused=None, violations=None, "
                     "status=None, returns=None)",
    "step": f"(p: {P}, state, action, out=None, reward=None, status=None)",
    "step_residual": f"(p: {P}, state, action, next_ref, partial=None)",
    "step_residual_blocks": "(n_transitions: int) -> int",
    "step_residual_normal_sets": f"(p_base: {P}, set_begin, max_set_len: int, points, state, action, next_ref, "
                                 "inv_2e=None, active=None, partial=None, out=None, status=None)",
    "step_residual_population": f"(p_base: {P}, cand, state, action, next_ref, partial=None, value=None, status=None)",
    "step_residual_sets": f"(p_base: {P}, set_begin, max_set_len: int, cand, cand_set, state, action, next_ref, "
                          "partial=None, value=None, status=None)",
    "traj_moments": f"(p: {P}, traj, acc=None)",
}
CONSTANTS = dict(CACLA_HIDDEN=12, LQR_MAX_STATE=4, LQR_MAX_ACTION=2, LQR_THRESHOLD_STEP=0, LQR_THRESHOLD_FIXED=1,
                 LQR_COST_INF=0, LQR_COST_2=1, LQR_COST_1=2, LQR_REFUSED=0, LQR_ADMITTED=1, LQR_NOTHING_YET=2)


def public_signatures(module):
    out = {}
    for name, obj in vars(module).items():
        if name.startswith("_") or getattr(obj, "__module__", None) != module.__name__:
            continue
        if inspect.isclass(obj):
            for m, f in vars(obj).items():
                if inspect.isfunction(f) and (not m.startswith("_") or m == "__init__"):
                    out[f"{name}.{m}"] = str(inspect.signature(f))
        elif inspect.isfunction(obj):
            out[name] = str(inspect.signature(obj))
    return out


def test_the_public_interface_is_the_parent_commits():
    got = public_signatures(k)
    assert sorted(got) == sorted(SIGNATURES)
    for name in SIGNATURES:
        assert got[name] == SIGNATURES[name], name
    for name, value in CONSTANTS.items():
        assert getattr(k, name) == value, name
    for name in ("SwParams", "check", "load", "ptr", "require_gpu", "stream_ptr", "_lib"):    # what callers reach
        assert hasattr(k, name), name                                                         # through the module
    assert k.SingleEnv.DOUBLES == 64 and k.SingleEnv.ACTION == 18
