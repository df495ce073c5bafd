// swimmer_safe_ars_ensemble.hip -- sw_safe_ars_rollouts_ensemble_f64: the exploration rollouts of MANY Basic_ARS /
// Safe_ARS AGENTS in one launch (sw_safe_ars_rollouts_multi_f64, swimmer_rollout_safe_multi.hip), every real step of a
// gated agent behind the one-step look-ahead in an ENSEMBLE of up to 64 simulators: the step is taken only where every
// member's cost stays within the simulator threshold.  A translation unit of its own: no existing code object depends
// on it.
//
// Where the members live.  The kernel is the lane body (swimmer_rollout_safe_lane.inc with SW_SAFE_MULTI 1 and
// SW_SAFE_ENSEMBLE 1: one sw::euler_step<N> with the member's constants, one with the real ones, the policy
// P + / - nu delta with NumPy's rounding) with a rollout in a GROUP of G lanes, G the smallest power of two >=
// n_member, instead of in one lane.  Lane j of a group holds the constants of member j % n_member -- derived in the
// kernel with sw::consts_of from the member's (l_i, m_i, k) and the real h and direction: the host's bits, and the bits
// safe_ars_multi_lane_kernel gives that simulator.  The six member-dependent doubles of sw::Consts (l, kl_nm, h_kl_nm,
// six_k_m, kl_m, c12) are in VGPRs; h, dirx and diry stay uniform.  So the same instructions look ahead in every member
// -- no loop over the members -- and every lane of a group runs the real step redundantly, with the same bits.
//
// The gate is one wave ballot (__builtin_amdgcn_ballot_w64) per step over every lane's `cost <= sim_thresh` (NaN
// refuses), cut to the group's first n_member lanes: all lanes of a group see the same bits, so a group takes the step
// or leaves the loop WHOLE, and no lane is missing from a ballot the rest of its group still reaches.  The bits at the
// first refused step are refusing_members.  worst_max is a running maximum per lane of its own member's admitted costs
// (no NaN among them: each is <= the threshold), reduced over the group ONCE behind the loop -- a maximum is exact in
// any order -- and both sit behind uniform branches: a launch without worst_max does not pay for it.
//
// A 64-thread workgroup (one wave) holds 64 / G rollouts; the grid is (ceil(2 n_dir G / 64), n_agent).  Surplus groups
// recompute the agent's last rollout and store nothing; only lane 0 of a group stores, with plain vector stores: no
// atomics and no hand-over between workgroups.  G is a run-time argument (its log2), so there are seven kernels, one
// per n = 2..8, and SW_FLAG_ROLLOUT_* has nothing to choose from: it is accepted and ignored.  NOT BUILT: a mirror-quad
// ensemble form for n = 3, a row form, more than 64 members (a second wave per rollout).
#include "swimmer_launch.h"

namespace {

// SafeArsMultiArgs (swimmer_launch.h) plus the members and the two ensemble records
struct SafeArsEnsembleArgs {
    const double *policy, *deltas;
    const int32_t *gated;
    const double *sims, *sim_thresh, *real_thresh;
    double *returns, *cost_trace, *cost_max;
    int32_t *first_refused, *violations, *status;
    double *worst_max;
    int64_t *refusing_members;
};

#define SW_SAFE_MULTI 1
#define SW_SAFE_ENSEMBLE 1
template <int N>
__global__ void __launch_bounds__(kWave)
safe_ars_ensemble_kernel(sw::Consts Cr, int64_t n_roll, int32_t H, int32_t n_member, int32_t log2_group,
                         SafeArsEnsembleArgs all, double nu, int32_t cost_kind, int32_t cost_index)
{
    // the per-agent view (swimmer_rollout_safe_multi.inc's names) and the lane's place: group -> rollout, lane -> member
    const int lane = threadIdx.x;
    const int group = lane >> log2_group, in_group = lane - (group << log2_group);
    const int64_t slot = (int64_t)blockIdx.x * (kWave >> log2_group) + group;
    const int64_t r = slot < n_roll ? slot : n_roll - 1;       // a surplus group recomputes the last rollout
    const bool owner = in_group == 0 && slot < n_roll;         // the one lane that stores
    // this group's members out of a wave ballot: bit e = the verdict of lane e of the group, which holds member e
    const uint64_t every_member = n_member == kWave ? ~0ull : (1ull << n_member) - 1;
    auto member_bits = [&](uint64_t ballot) { return (ballot >> (group << log2_group)) & every_member; };

    const int64_t agent = blockIdx.y;
    const bool gated = __builtin_amdgcn_readfirstlane(all.gated[agent]) != 0;
    const double *__restrict__ const policies = all.policy + agent * ((N - 1) * (2 * N + 2));
    const double *__restrict__ const deltas = all.deltas + agent * (n_roll >> 1) * ((N - 1) * (2 * N + 2));
    double *__restrict__ const returns = all.returns + agent * n_roll;
    double *__restrict__ const cost_max = all.cost_max ? all.cost_max + agent * n_roll : nullptr;
    int32_t *__restrict__ const first_refused = all.first_refused ? all.first_refused + agent * n_roll : nullptr;
    int32_t *__restrict__ const violations = all.violations ? all.violations + agent * n_roll : nullptr;
    int32_t *__restrict__ const status = all.status ? all.status + agent * n_roll : nullptr;
    double *const worst_max = all.worst_max ? all.worst_max + agent * n_roll : nullptr;
    int64_t *const refusing_members = all.refusing_members ? all.refusing_members + agent * n_roll : nullptr;
    double *const traj = nullptr;
    const double real_thresh = uniform_f64(all.real_thresh[agent]);
    double sim_thresh = 0.0;
    sw::Consts Cs = Cr;       // an ungated agent's: never used
    if (gated) {   // uniform: an ungated agent reads neither sims nor sim_thresh
        const double *const sm = all.sims + (agent * n_member + in_group % n_member) * 3;
        const double sim_l = sm[0], sim_m = sm[1], sim_k = sm[2];
        const uint64_t bad = __builtin_amdgcn_ballot_w64(!sim_params_ok(sim_l, sim_m, sim_k));
        if (bad) {   // uniform: every group holds the same members.  The convention of sw_safe_ars_rollouts_multi_f64
            if (owner) {
                returns[r] = __builtin_nan("");
                if (status) status[r] = SW_STATUS_PARAM;
                if (first_refused) first_refused[r] = 0;
                if (violations) violations[r] = 0;
                if (cost_max) cost_max[r] = __builtin_nan("");
                if (all.cost_trace)
                    for (int32_t t = 0; t < H; ++t)
                        all.cost_trace[((int64_t)t * gridDim.y + agent) * n_roll + r] = __builtin_nan("");
                if (worst_max) worst_max[r] = __builtin_nan("");
                if (refusing_members) refusing_members[r] = (int64_t)member_bits(bad);
            }
            return;
        }
        Cs = sw::consts_of(N, sim_l, sim_m, sim_k, Cr.h, Cr.dirx, Cr.diry);   // per lane: the member's, in VGPRs
        sim_thresh = uniform_f64(all.sim_thresh[agent]);
    }
    const sw::Consts Creal = Cr, Csim = Cs;   // the lane body's names
    const bool want_worst = worst_max != nullptr;
    double worst = 0.0;                        // this lane's member: its largest admitted cost (costs are >= 0)
    uint64_t refusing = 0;                     // the members that refused the first refused step
#include "swimmer_rollout_safe_lane.inc"
    if (want_worst) {   // uniform; every lane of the wave is here again
        if (gated)      // uniform
            for (int s = 1; s < (1 << log2_group); s <<= 1) worst = fmax(worst, __shfl_xor(worst, s));
        if (owner) worst_max[r] = gated ? worst : __builtin_nan("");
    }
    if (owner && refusing_members) refusing_members[r] = (int64_t)refusing;
}
#undef SW_SAFE_ENSEMBLE
#undef SW_SAFE_MULTI

}  // namespace

int sw_safe_ars_rollouts_ensemble_f64(const sw_params *real, int64_t n_agent, int32_t n_member, int64_t n_dir, int32_t H,
                                      const double *policy, const double *deltas, double nu, const int32_t *gated,
                                      const double *sims, const double *sim_thresh, const double *real_thresh,
                                      int32_t cost_kind, int32_t cost_index, double *returns, double *cost_trace,
                                      double *cost_max, int32_t *first_refused, int32_t *violations, int32_t *status,
                                      double *worst_max, int64_t *refusing_members, void *stream)
{
    int rc = check_params(real);
    if (rc) return rc;
    // the size rule of the multi-agent launches: grid.y = agent, rollouts indexed like a single launch's
    if (n_agent < 1 || n_agent > 65535 || n_dir < 1 || n_dir > ((int64_t)1 << 23) || H < 0) return SW_ERR_SIZE;
    if (n_member < 1 || n_member > kWave) return SW_ERR_SIZE;   // the members ride in one wave's lanes
    if ((rc = check_cost(real, cost_kind, cost_index)) != SW_OK) return rc;
    if (!policy || !deltas || !gated || !sims || !sim_thresh || !real_thresh || !returns) return SW_ERR_NULL;
    int32_t log2_group = 0;
    while ((1 << log2_group) < n_member) ++log2_group;
    const int64_t n_roll = 2 * n_dir, per_block = kWave >> log2_group;
    const dim3 grid((unsigned)((n_roll + per_block - 1) / per_block), (unsigned)n_agent);
    if ((int64_t)grid.x * grid.y * kWave >= ((int64_t)1 << 32)) return SW_ERR_SIZE;
    if (is_twin(real)) return SW_ERR_PARAM;
    const SafeArsEnsembleArgs a{policy,   deltas,        gated,      sims,   sim_thresh, real_thresh,     returns, cost_trace,
                                cost_max, first_refused, violations, status, worst_max,  refusing_members};
    const bool known_n = with_n<2, 8>(real->n, [&](auto N) {
        hipLaunchKernelGGL((safe_ars_ensemble_kernel<N.value>), grid, dim3(kWave), 0, (hipStream_t)stream,
                           make_consts(real), n_roll, H, n_member, log2_group, a, nu, cost_kind, cost_index);
    });
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}
