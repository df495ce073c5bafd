// swimmer_rollout_lane.hip -- rollouts with ONE ROLLOUT PER LANE (any n, either model): the throughput form for
// batches that fill the chip, with its ARS gate and safe-exploration kernels.
#include "swimmer_launch.h"

namespace {

// ------------------------------------------------------------------------------------
// Rollouts.  ARS = false: policies[r][m][d] given per rollout.  ARS = true: rollout r is
// direction dir_begin + (r >> 1) with sign + (r even) / - (r odd); its policy
// P +- nu * delta is built here (ars_agent.py:141-142), so the perturbed policies never
// exist in HBM.  The V2 whitening P diag(inv_std) (ars/environment.py:32-33) is folded into
// the register copy of the policy once per rollout instead of once per step.
template <int N, bool ARS, bool TWIN>
__global__ void __launch_bounds__(kRollBlock)
rollout_kernel(sw::Consts C, sw::TwinConsts T, int64_t n_roll, int32_t H, const double *__restrict__ policies,
               const double *__restrict__ deltas, int64_t dir_begin, double nu,
               const double *__restrict__ mean, const double *__restrict__ inv_std,
               const double *__restrict__ state0, double *__restrict__ returns,
               double *__restrict__ traj, double *__restrict__ final_state,
               double *__restrict__ moments, int32_t *__restrict__ status)
{
#define SW_GATE_BODY 0
#include "swimmer_rollout_lane.inc"
#undef SW_GATE_BODY
}

// The ARS simulator gate (sw_ars_gate_f64) in the lane form: one rollout per lane, any n, either model.
// The body is rollout_kernel's (swimmer_rollout_lane.inc) with ARS on, no trajectories / final state /
// moments, and the decision (gate_store) in place of the plain return store.
template <int N, bool TWIN>
__global__ void __launch_bounds__(kRollBlock)
ars_gate_kernel(sw::Consts C, sw::TwinConsts T, int64_t n_roll, int32_t H, const double *__restrict__ policies,
                const double *__restrict__ deltas, int64_t dir_begin, double nu,
                const double *__restrict__ mean, const double *__restrict__ inv_std, double gate_thr,
                int32_t *__restrict__ admit, double *__restrict__ returns, int32_t *__restrict__ status)
{
    constexpr bool ARS = true;
    const double *const state0 = nullptr;
    double *const traj = nullptr;
    double *const final_state = nullptr;
    double *const moments = nullptr;
#define SW_GATE_BODY 1
#include "swimmer_rollout_lane.inc"
#undef SW_GATE_BODY
}

// sw_ars_rollouts_multi_f64 in the lane form (any n, either model): the ARS rollouts of many agents in one launch,
// the lane body behind the per-agent view (swimmer_rollout_multi.inc).  An agent's rollouts fill whole 64-lane
// workgroups of their own; the lanes behind its last rollout idle.
#define SW_MULTI_N N
template <int N, bool TWIN>
__global__ void __launch_bounds__(kRollBlock)
ars_multi_lane_kernel(sw::Consts C, sw::TwinConsts T, int64_t n_roll, int32_t H, sw_launch::MultiArgs all, double nu)
{
    constexpr bool ARS = true;
#include "swimmer_rollout_multi.inc"
#define SW_GATE_BODY 0
#include "swimmer_rollout_lane.inc"
#undef SW_GATE_BODY
}

// sw_ars_gate_multi_f64 and sw_ars_rollouts_multi_counted_f64 in the lane form (the view's header has the two modes).
// The twin model's constants of an agent's simulator are its (l_i, m_i, k) as they are.
#define SW_MULTI_SLOTS kRollBlock
#define SW_MULTI_GATE 1
template <int N, bool TWIN>
__global__ void __launch_bounds__(kRollBlock)
ars_gate_multi_lane_kernel(sw::Consts base, int64_t n_roll, int32_t H, sw_launch::SafeMultiArgs all, double nu)
{
    constexpr bool ARS = true;
#include "swimmer_rollout_multi.inc"
    const sw::TwinConsts T{sim_l, sim_m, sim_k, base.h, base.dirx, base.diry};
#define SW_GATE_BODY 1
#include "swimmer_rollout_lane.inc"
#undef SW_GATE_BODY
}

// The member launch of sw_ars_gate_ensemble_f64 in the lane form: the same body behind the view with
// SW_MULTI_ENSEMBLE 1 (blockIdx.y = agent * n_sim + member).
#define SW_MULTI_ENSEMBLE 1
template <int N, bool TWIN>
__global__ void __launch_bounds__(kRollBlock)
ars_gate_ens_lane_kernel(sw::Consts base, int64_t n_roll, int32_t H, sw_launch::EnsembleArgs all, double nu)
{
    constexpr bool ARS = true;
#include "swimmer_rollout_multi.inc"
    const sw::TwinConsts T{sim_l, sim_m, sim_k, base.h, base.dirx, base.diry};
#define SW_GATE_BODY 1
#include "swimmer_rollout_lane.inc"
#undef SW_GATE_BODY
}
#undef SW_MULTI_ENSEMBLE
#undef SW_MULTI_GATE

#define SW_MULTI_COUNTED 1
template <int N, bool TWIN>
__global__ void __launch_bounds__(kRollBlock)
ars_counted_lane_kernel(sw::Consts C, sw::TwinConsts T, int64_t n_roll_max, int32_t H, sw_launch::SafeMultiArgs all,
                        double nu)
{
    constexpr bool ARS = true;
#include "swimmer_rollout_multi.inc"
#define SW_GATE_BODY 0
#include "swimmer_rollout_lane.inc"
#undef SW_GATE_BODY
}
#undef SW_MULTI_COUNTED
#undef SW_MULTI_SLOTS
#undef SW_MULTI_N

// ------------------------------------------------------------------------------------
// Safe exploration (safe_ars/ars.py:101-153): every real step of a rollout is gated by a ONE-STEP look-ahead in a
// simulator -- `isSafe` = sim_env.set_state(obs) + sim_env.step(action) + cost(sim obs) <= sim_thresh (:111-122,
// called at :141).  One rollout per lane, the whole H-step loop in one launch: per step the action (policy @ obs,
// :139), one Euler step with the SIMULATOR's constants on a copy of the state, the cost of where that lands, and --
// if the gate is open -- the real step.  A refused step leaves the real env where it is (:150-151), so the same
// action is proposed and refused for the rest of the horizon: the lane stops stepping and only repeats its state
// into the trajectory.  Costs (include/swimmer_hip.h SW_COST_*): |obs[j]|, or max_i |thetadot_i| (the reference's
// own experiment, safe_ars/experiment.py:45).
template <int N>
__global__ void __launch_bounds__(kRollBlock)
safe_rollout_kernel(sw::Consts Creal, sw::Consts Csim, int64_t n_roll, int32_t H,
                    const double *__restrict__ policies, int32_t cost_kind, int32_t cost_index,
                    double sim_thresh, double real_thresh, double *__restrict__ returns,
                    double *__restrict__ traj, int32_t *__restrict__ first_refused,
                    int32_t *__restrict__ violations, int32_t *__restrict__ status)
{
#define SW_SAFE_MULTI 0
#include "swimmer_rollout_safe_lane.inc"
#undef SW_SAFE_MULTI
}

// ---- host: the form's launch functions (private) and its table of them (sw_launch) ----
using namespace sw_launch;

int launch_lane(const sw_params *p, const RolloutPlan &plan, bool ars, int64_t n_roll, int32_t H, const RolloutArgs &a,
                hipStream_t stream, const SideWork *)
{
    const sw::Consts C = make_consts(p);
    const sw::TwinConsts T = make_twin_consts(p);
    const bool known_n = with_n<2, 8>(p->n, [&](auto N, auto ARS, auto TWIN) {
        hipLaunchKernelGGL((rollout_kernel<N.value, ARS.value, TWIN.value>), dim3(plan.rollout_blocks),
                           dim3(plan.block), 0, stream, C, T, n_roll, H, a.policies, a.deltas, a.dir_begin,
                           a.nu, a.mean, a.inv_std, a.state0, a.returns, a.traj, a.final_state, a.moments,
                           a.status);
    }, ars, is_twin(p));
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

int launch_gate_lane(const sw_params *sim, const RolloutPlan &plan, int64_t n_roll, int32_t H, const RolloutArgs &a,
                     double gate_thr, int32_t *admit, hipStream_t stream)
{
    const sw::Consts C = make_consts(sim);
    const sw::TwinConsts T = make_twin_consts(sim);
    const bool known_n = with_n<2, 8>(sim->n, [&](auto N, auto TWIN) {
        hipLaunchKernelGGL((ars_gate_kernel<N.value, TWIN.value>), dim3(plan.rollout_blocks), dim3(plan.block), 0,
                           stream, C, T, n_roll, H, a.policies, a.deltas, a.dir_begin, a.nu, a.mean, a.inv_std,
                           gate_thr, admit, a.returns, a.status);
    }, is_twin(sim));
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

int launch_multi_lane(const sw_params *p, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, int32_t H,
                      const MultiArgs &a, double nu, hipStream_t stream)
{
    const sw::Consts C = make_consts(p);
    const sw::TwinConsts T = make_twin_consts(p);
    const bool known_n = with_n<2, 8>(p->n, [&](auto N, auto TWIN) {
        launch_agent_grid(ars_multi_lane_kernel<N.value, TWIN.value>, plan, n_agent, n_roll, stream, C, T, n_roll, H, a,
                          nu);
    }, is_twin(p));
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

int launch_gate_multi_lane(const sw_params *p, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, int32_t H,
                           const SafeMultiArgs &a, double nu, hipStream_t stream)
{
    const bool known_n = with_n<2, 8>(p->n, [&](auto N, auto TWIN) {
        launch_agent_grid(ars_gate_multi_lane_kernel<N.value, TWIN.value>, plan, n_agent, n_roll, stream,
                          make_consts(p), n_roll, H, a, nu);
    }, is_twin(p));
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

int launch_gate_ens_lane(const sw_params *p, const RolloutPlan &plan, int64_t n_member, int64_t n_roll, int32_t H,
                         const EnsembleArgs &a, double nu, hipStream_t stream)
{
    const bool known_n = with_n<2, 8>(p->n, [&](auto N, auto TWIN) {
        launch_agent_grid(ars_gate_ens_lane_kernel<N.value, TWIN.value>, plan, n_member, n_roll, stream,
                          make_consts(p), n_roll, H, a, nu);
    }, is_twin(p));
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

int launch_counted_lane(const sw_params *p, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, int32_t H,
                        const SafeMultiArgs &a, double nu, hipStream_t stream)
{
    const sw::Consts C = make_consts(p);
    const sw::TwinConsts T = make_twin_consts(p);
    const bool known_n = with_n<2, 8>(p->n, [&](auto N, auto TWIN) {
        launch_agent_grid(ars_counted_lane_kernel<N.value, TWIN.value>, plan, n_agent, n_roll, stream, C, T, n_roll, H,
                          a, nu);
    }, is_twin(p));
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

int launch_safe_lane(const sw_params *real, const sw_params *sim, const RolloutPlan &plan, int64_t n_roll, int32_t H,
                     const double *policies, int32_t cost_kind, int32_t cost_index, double sim_thresh,
                     double real_thresh, double *returns, double *traj, int32_t *first_refused, int32_t *violations,
                     int32_t *status, hipStream_t stream)
{
    const sw::Consts Cr = make_consts(real), Cs = make_consts(sim);
    const bool known_n = with_n<2, 8>(real->n, [&](auto N) {
        hipLaunchKernelGGL((safe_rollout_kernel<N.value>), dim3(plan.rollout_blocks), dim3(plan.block), 0, stream, Cr,
                           Cs, n_roll, H, policies, cost_kind, cost_index, sim_thresh, real_thresh, returns, traj,
                           first_refused, violations, status);
    });
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}
SafeArsMultiLauncher launch_safe_ars_multi_lane;   // swimmer_rollout_safe_multi.hip, later in the translation unit

}  // namespace

namespace sw_launch __attribute__((visibility("hidden"))) {
FormLaunchers kLaneLaunchers = {launch_lane,         launch_gate_lane, launch_multi_lane, launch_gate_multi_lane,
                                launch_counted_lane, launch_safe_lane, launch_safe_ars_multi_lane,
                                launch_gate_ens_lane};
}  // namespace sw_launch
