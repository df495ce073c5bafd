// swimmer_cacla_gated.h -- the run loop of CACLA on the swimmer BEHIND A SIMULATOR GATE, one body for the gate in one
// simulator (swimmer_cacla_safe.hip, sw_cacla_safe_run_f64) and in an ensemble of them (swimmer_cacla_ensemble.hip,
// sw_cacla_safe_ensemble_run_f64): the learner of swimmer_cacla_learner.h (cacla/cacla_agent.py:165-190; its header
// explains layout and summation order) inside the run loop of the reference's safe agents
// (cacla/cacla_safe_agent.py:161-188), every real step gated by a one-step look-ahead (safe_ars/ars.py:111-122).  Whole
// runs of MANY INDEPENDENT AGENTS in one launch, one wave per agent.
//
// cacla::gated_kernel<N, ENSEMBLE> is a __global__ template that each of the two units instantiates for itself; the two
// forms differ where ENSEMBLE is tested below -- the simulator's constants, `admit`, mem_ok, n_out, the worst-cost record
// and the members' refusal counts -- and nowhere else.  NOT a __device__ function behind two thin kernels: that form
// was built and costs registers in every one of the 14 kernels (swimmer_cacla_learner.h has the figures).  Two contracts follow from the one body, and tests/test_cacla_safe_gpu.py and test_cacla_ensemble_gpu.py
// hold the kernels to them at every n:
//   * an UNGATED agent (gated[a] == 0: no look-ahead, every step taken) runs the learner's pieces in cacla_kernel's
//     order and so has the bits of sw_cacla_run_f64(train = 1);
//   * an ensemble of one member, or of copies of one simulator, has the bits of the single-simulator kernel.
//
// One step of a gated agent: FA_act = actors(state), action = FA_act + noise[t] (consumed whether or not the step is
// taken); the look-ahead from the same state with the same action (sw::euler_step with the simulator's constants,
// derived here with sw::consts_of: the host's bits); in = cost(sim_state) <= sim_thresh (NaN refuses).  The real step
// with the learner's update behind it is a uniform branch.  A refused step changes nothing.  Lane t & 63 keeps step t's
// reward entry (the last admitted step's reward, NaN before the first admission), its admit flag and, in an ensemble,
// its worst cost; they are stored once per 64-step block.
//
// Where the simulators live.  ONE SIMULATOR: every lane runs the look-ahead redundantly with the agent's constants in
// scalar registers, so `in` is the same in all of them and `admit` is the first lane's, in a scalar register; a
// simulator that breaks the parameter rule refuses every step without a look-ahead.  AN ENSEMBLE: lane L holds the
// constants of member L % n_member, so the same instructions look ahead in every member.  The six member-dependent
// doubles of sw::Consts (l, kl_nm, h_kl_nm, six_k_m, kl_m, c12) are in VGPRs; h, dirx and diry stay uniform.  Every
// lane is active in the look-ahead, and with n_member < 64 members repeat: no lane is masked.  `in` is false in the
// lanes of a member that breaks the parameter rule, which look ahead with the real constants and not with the
// member's; admit = every lane's `in`, through a wave ballot into scalar registers.  MORE THAN 64 MEMBERS (a second
// wave per agent) IS NOT BUILT.
//
// The two optional records of an ensemble.  worst_rec[t] = max over the lanes of (in-range cost, NaN or a bad member ->
// +inf): the map comes first, and a maximum of non-NaN doubles is exact in any order, so the reduction (four DPP steps
// inside a 16-lane row, then the four rows through scalar registers) needs no order contract.  It sits behind a uniform
// branch: a launch without worst_rec does not pay for it.  member_refusals[e]: lane e < n_member counts the steps at
// which its own `in` was false, one VALU add per step, and adds the count to memory at the end.
#pragma once
#include "swimmer_cacla_learner.h"

namespace {
namespace cacla {

constexpr int kGatedBlock = kWave;   // one wave per agent, one workgroup per wave

// An entry point's arrays.  sims: [n_agent][n_member][3], [n_agent][3] for the single simulator, whose struct is the
// ensemble's without the two records.  Two structs, not the superset with null records: behind the superset the
// single-simulator kernels at n <= 5 keep fewer scalars in spill lanes and come out with another step loop (34 .. 43
// instructions shorter); with its own struct every kernel has the loop it had before the two were merged.
template <bool ENSEMBLE> struct GatedArgs;
template <> struct GatedArgs<false> {
    const double *gamma, *alpha, *noise;
    const int32_t *gated;
    const double *sims, *sim_thresh, *real_thresh;
    double *weights, *state, *last_reward, *rewards;
    int32_t *admitted_rec, *counters, *first_refused, *status;
};
template <> struct GatedArgs<true> {
    const double *gamma, *alpha, *noise;
    const int32_t *gated;
    const double *sims, *sim_thresh, *real_thresh;
    double *weights, *state, *last_reward, *rewards;
    int32_t *admitted_rec;
    double *worst_rec;
    int32_t *member_refusals, *counters, *first_refused, *status;
};

// v of the lane a DPP control names (one every lane of the wave has: the controls below are permutations of a row)
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// The largest v of the wave in every lane; v is not NaN in any lane (the caller maps NaN to +inf first), so the order
// does not matter.  Lanes 1, 2 (quad_perm), 4 (row_half_mirror) and 8 (row_mirror) apart inside a 16-lane row, then the
// four rows' values through scalar registers.
__device__ __forceinline__ double wave_max_f64(double v)
{
    v = fmax(v, dpp_f64<1 | (0 << 2) | (3 << 4) | (2 << 6)>(v));   // quad_perm [1,0,3,2]
    v = fmax(v, dpp_f64<2 | (3 << 2) | (0 << 4) | (1 << 6)>(v));   // quad_perm [2,3,0,1]
    v = fmax(v, dpp_f64<0x141>(v));                                // row_half_mirror: lane 7 - i of each eight
    v = fmax(v, dpp_f64<0x140>(v));                                // row_mirror: lane 15 - i of the row
    return fmax(fmax(lane_value(v, 0), lane_value(v, 16)), fmax(lane_value(v, 32), lane_value(v, 48)));
}

template <int N, bool ENSEMBLE>
__global__ void __launch_bounds__(kGatedBlock)
gated_kernel(sw::Consts C, int32_t n_member, int32_t n_iter, int32_t t_begin, int32_t cost_kind, int32_t cost_index,
             GatedArgs<ENSEMBLE> a)
{
    using S = Shape<N>;
    constexpr int D = S::D, M = S::M, UPL = S::UPL;
    constexpr unsigned long long kEveryLane = ~0ull;
    __shared__ double prod[2][kWave * UPL];            // products of the forward at s (0) and at s' (1)

    const int lane = threadIdx.x;
    const int64_t agent = blockIdx.x;
    const Place pl = place_of<N>(lane);

    double *const wn = a.weights + (agent * N + pl.net) * S::NETD;
    double W1[UPL][D], b1[UPL], W2[UPL], b2;
    load_weights<N>(wn, pl.j0, W1, b1, W2, b2);

    double *const sp = a.state + agent * D;
    double gdx, gdy, th[N], thd[N];
    load_state<N>(sp, gdx, gdy, th, thd);
    const double gam = a.gamma[agent], alp = a.alpha[agent];

    // the gate: whether there is one (wave-uniform, like the thresholds), and the simulator -- the agent's, or THIS
    // LANE's member
    const bool gated = __builtin_amdgcn_readfirstlane(a.gated[agent]) != 0;
    const double real_thresh = uniform_f64(a.real_thresh[agent]);
    double sim_thresh = 0.0;
    sw::Consts Cs = C;        // a bad member's lanes keep the real constants: its own are not used
    bool mem_ok = true;       // this lane's simulator satisfies the parameter rule
    bool sim_ok = true;       // every simulator of the agent does (uniform)
    if (gated) {   // uniform: an ungated agent reads neither sims nor sim_thresh
        const double *const sm = a.sims + (ENSEMBLE ? agent * n_member + lane % n_member : agent) * 3;
        const double sim_l = sm[0], sim_m = sm[1], sim_k = sm[2];
        mem_ok = sim_params_ok(sim_l, sim_m, sim_k);
        if constexpr (ENSEMBLE) {
            if (mem_ok) Cs = sw::consts_of(N, sim_l, sim_m, sim_k, C.h, C.dirx, C.diry);
            sim_ok = __builtin_amdgcn_ballot_w64(mem_ok) == kEveryLane;
        } else {
            sim_ok = __builtin_amdgcn_readfirstlane(mem_ok ? 1 : 0) != 0;
            if (sim_ok) Cs = uniform_consts(sw::consts_of(N, sim_l, sim_m, sim_k, C.h, C.dirx, C.diry));
        }
        sim_thresh = uniform_f64(a.sim_thresh[agent]);
    }

    const double *const np = a.noise + agent * (int64_t)n_iter * M;
    double nz[M], nz_next[M];
    load_noise<N>(np, n_iter, 0, lane, nz);

    double *const rp = a.rewards + agent * (int64_t)n_iter;
    int32_t *const ap = a.admitted_rec ? a.admitted_rec + agent * (int64_t)n_iter : nullptr;
    double *wp = nullptr;
    if constexpr (ENSEMBLE) wp = a.worst_rec ? a.worst_rec + agent * (int64_t)n_iter : nullptr;
    double last = uniform_f64(a.last_reward[agent]);     // the reward entry of a refused step
    // worst (a step's entry of worst_rec) and n_out are the ensemble's alone and dead with one simulator.  They are
    // declared HERE, among the stages: declared behind refused_at, or worst inside the step loop, they reorder the
    // loops' phis in the single-simulator kernels and with them the schedule of the n = 7 step loop.
    double rstage = 0.0, wstage = 0.0, worst;
    int32_t astage = 0;
    int32_t n_out = 0;        // per lane: the steps at which this lane's member did not admit
    bool ok = true;
    double thmax = 0.0;
    int32_t n_upd = 0, n_adm = 0, n_viol = 0, refused_at = -1;

    for (int32_t t0 = 0; t0 < n_iter; t0 += kWave) {
        load_noise<N>(np, n_iter, t0 + kWave, lane, nz_next);   // a block ahead: consumed 64 steps from here
        const int32_t steps = (n_iter - t0 < kWave) ? n_iter - t0 : kWave;
        for (int32_t k = 0; k < steps; ++k) {
            thmax = sw::track_angle_range<N>(thmax, th);
            double x[D], h[UPL], out[N], act[M];
            bool off[UPL];
            observe<N>(gdx, gdy, th, thd, x);
            forward<N>(prod[0], pl, W1, b1, W2, b2, x, h, off, out);
#pragma unroll
            for (int i = 0; i < M; ++i) act[i] = __dadd_rn(out[i], lane_value(nz[i], k));   // mean + noise

            bool admit = true;
            if constexpr (ENSEMBLE) worst = __builtin_nan("");   // an ungated agent's entry
            if (gated) {   // uniform: the look-ahead from the real state (cacla_safe_agent.py:166-168)
                admit = false;
                if (ENSEMBLE || sim_ok) {   // uniform; every member looks ahead, each in its lanes
                    double sgx = gdx, sgy = gdy, sth[N], sthd[N], srew;
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        sth[i] = th[i];
                        sthd[i] = thd[i];
                    }
                    (void)sw::euler_step<N>(Cs, sgx, sgy, sth, sthd, act, srew);
                    const double c = safe_cost<N>(cost_kind, cost_index, sgx, sgy, sth, sthd);
                    if constexpr (ENSEMBLE) {
                        const bool in = mem_ok && c <= sim_thresh;   // NaN refuses, and so does a bad member
                        n_out += in ? 0 : 1;
                        admit = __builtin_amdgcn_ballot_w64(in) == kEveryLane;   // every member admits: a scalar
                        if (wp) worst = wave_max_f64((mem_ok && c == c) ? c : __builtin_inf());   // uniform
                    } else {
                        const bool in = c <= sim_thresh;   // NaN refuses
                        admit = __builtin_amdgcn_readfirstlane(in ? 1 : 0) != 0;   // every lane holds the same: lane 0's
                    }
                }
            }
            if (admit) {   // uniform
                double rew;
                ok = sw::euler_step<N>(C, gdx, gdy, th, thd, act, rew) && ok;
                n_adm += 1;
                n_viol += (safe_cost<N>(cost_kind, cost_index, gdx, gdy, th, thd) > real_thresh) ? 1 : 0;
                last = rew;
                learn<N>(prod[1], pl, W1, b1, W2, b2, gdx, gdy, th, thd, x, h, off, out, act, rew, gam, alp, n_upd);
            } else {
                refused_at = (refused_at < 0) ? t0 + k : refused_at;
            }
            rstage = (lane == k) ? last : rstage;
            astage = (lane == k) ? (admit ? 1 : 0) : astage;
            if constexpr (ENSEMBLE) wstage = (lane == k) ? worst : wstage;
        }
        if (lane < steps) {                              // one coalesced store each per block (the last one partial)
            rp[t0 + lane] = rstage;
            if (ap) ap[t0 + lane] = astage;
            if (wp) wp[t0 + lane] = wstage;
        }
#pragma unroll
        for (int i = 0; i < M; ++i) nz[i] = nz_next[i];
    }

    if (pl.valid) store_weights<N>(wn, pl.j0, W1, b1, W2, b2);
    if constexpr (ENSEMBLE) {
        if (gated && a.member_refusals && lane < n_member)   // lane e < n_member holds member e
            a.member_refusals[agent * n_member + lane] += n_out;
    }
    if (lane == 0) {
        const bool fin = store_state<N>(sp, gdx, gdy, th, thd);
        if (a.status)
            a.status[agent] |= (ok ? 0 : SW_STATUS_SINGULAR) | (fin ? 0 : SW_STATUS_NONFINITE) |
                               (thmax < sw::kAngleLimit ? 0 : SW_STATUS_RANGE) | (sim_ok ? 0 : SW_STATUS_PARAM);
        a.last_reward[agent] = last;
        a.counters[agent * 3] += n_adm;
        a.counters[agent * 3 + 1] += n_viol;
        a.counters[agent * 3 + 2] += n_upd;
        if (refused_at >= 0 && a.first_refused[agent] < 0) a.first_refused[agent] = t_begin + refused_at;
    }
}

// The two entry points behind their argument lists: the argument check in the order both always had (the entry-code
// tests pin it; n_member is 1 from the single-simulator entry), then one launch of gated_kernel<real->n, ENSEMBLE>,
// instantiated by the unit that calls this.
template <bool ENSEMBLE>
int gated_run(const sw_params *real, int64_t n_agent, int32_t n_member, int32_t n_iter, int64_t t_begin,
              int32_t cost_kind, int32_t cost_index, const GatedArgs<ENSEMBLE> &a, void *stream)
{
    int rc = check_params(real);
    if (rc) return rc;
    if (!a.gamma || !a.alpha || !a.noise || !a.gated || !a.sims || !a.sim_thresh || !a.real_thresh || !a.weights ||
        !a.state || !a.last_reward || !a.rewards || !a.counters || !a.first_refused)
        return SW_ERR_NULL;
    if (n_agent < 1 || n_agent > INT32_MAX || n_iter < 0) return SW_ERR_SIZE;   // grid.x: one workgroup per agent
    if (n_member < 1 || n_member > kWave) return SW_ERR_SIZE;                   // the members ride in one wave's lanes
    if (t_begin < 0 || t_begin > (int64_t)INT32_MAX - n_iter) return SW_ERR_SIZE;   // first_refused is an int32 step
    if ((rc = check_cost(real, cost_kind, cost_index)) != SW_OK) return rc;
    if (is_twin(real)) return SW_ERR_PARAM;
    if (n_iter == 0) return SW_OK;
    const sw::Consts C = make_consts(real);
    const bool known_n = with_n<2, 8>(real->n, [&](auto N) {
        hipLaunchKernelGGL((gated_kernel<N.value, ENSEMBLE>), dim3((unsigned)n_agent), dim3(kGatedBlock), 0,
                           (hipStream_t)stream, C, n_member, n_iter, (int32_t)t_begin, cost_kind, cost_index, a);
    });
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

}  // namespace cacla
}  // namespace
