// swimmer_rollout_safe_multi.hip -- sw_safe_ars_rollouts_multi_f64: the per-step simulator gate (safe_ars/ars.py
// Safe_ARS.rollout) and the ungated Basic_ARS.rollout for the 2N exploration rollouts of MANY AGENTS in one launch --
// what safe_ars/experiment.py trains, a basic and a safe agent per seed.  Each kernel is its form's safe body
// (swimmer_rollout_safe_oct3.inc, swimmer_rollout_safe_lane.inc with SW_SAFE_MULTI 1) behind the per-agent view
// (swimmer_rollout_safe_multi.inc): per rollout the arithmetic of sw_safe_rollouts_f64 in the same form on the policy
// P + / - nu delta, the look-ahead skipped for an ungated agent.  No trajectory: the experiment reads its states as
// cost(state) only, so the kernels write that one number per rollout and step (cost_trace) and its maximum.
#include "swimmer_launch.h"
#include "swimmer_oct3.h"

namespace {

// n = 3, mirror-quad form: 16 rollout slots per 128-thread workgroup.  COST: a cost trace or a cost maximum is asked for.
#define SW_MULTI_N 3
#define SW_MULTI_SLOTS kMomGroup
template <bool COST, bool VIOL>
__global__ void __launch_bounds__(kOctBlock)
safe_ars_multi_oct3_kernel(sw::Consts Cr, int64_t n_roll, int32_t H, sw_launch::SafeArsMultiArgs all, double nu,
                           int32_t cost_kind, int32_t cost_index)
{
    constexpr bool TRAJ = false;
#include "swimmer_rollout_safe_multi.inc"
#define SW_SAFE_MULTI 1
#include "swimmer_rollout_safe_oct3.inc"
#undef SW_SAFE_MULTI
}
#undef SW_MULTI_SLOTS
#undef SW_MULTI_N

// any n = 2..8, one rollout per lane: 64 slots per workgroup
#define SW_MULTI_N N
#define SW_MULTI_SLOTS kRollBlock
template <int N>
__global__ void __launch_bounds__(kRollBlock)
safe_ars_multi_lane_kernel(sw::Consts Cr, int64_t n_roll, int32_t H, sw_launch::SafeArsMultiArgs all, double nu,
                           int32_t cost_kind, int32_t cost_index)
{
#include "swimmer_rollout_safe_multi.inc"
#define SW_SAFE_MULTI 1
#include "swimmer_rollout_safe_lane.inc"
#undef SW_SAFE_MULTI
}
#undef SW_MULTI_SLOTS
#undef SW_MULTI_N

// ---- host: the safe_ars_multi entries of the tables in swimmer_rollout_n3.hip and swimmer_rollout_lane.hip ----
using namespace sw_launch;

int launch_safe_ars_multi_oct3(const sw_params *real, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll,
                               int32_t H, const SafeArsMultiArgs &a, double nu, int32_t cost_kind, int32_t cost_index,
                               hipStream_t stream)
{
    with_bools([&](auto COST, auto VIOL) {
        launch_agent_grid(safe_ars_multi_oct3_kernel<COST.value, VIOL.value>, plan, n_agent, n_roll, stream,
                          make_consts(real), n_roll, H, a, nu, cost_kind, cost_index);
    }, a.cost_trace != nullptr || a.cost_max != nullptr, a.violations != nullptr);
    return launch_status();
}

int launch_safe_ars_multi_lane(const sw_params *real, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll,
                               int32_t H, const SafeArsMultiArgs &a, double nu, int32_t cost_kind, int32_t cost_index,
                               hipStream_t stream)
{
    const bool known_n = with_n<2, 8>(real->n, [&](auto N) {
        launch_agent_grid(safe_ars_multi_lane_kernel<N.value>, plan, n_agent, n_roll, stream, make_consts(real), n_roll,
                          H, a, nu, cost_kind, cost_index);
    });
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

}  // namespace
