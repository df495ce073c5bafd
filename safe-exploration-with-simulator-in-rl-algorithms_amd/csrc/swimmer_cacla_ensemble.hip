// swimmer_cacla_ensemble.hip -- CACLA on the swimmer, every real step gated on an ENSEMBLE of simulators: the run loop
// of cacla_safe_kernel (swimmer_cacla_safe.hip; the learner of swimmer_cacla_learner.h, its pieces in the same order)
// with the one-step look-ahead in up to 64 simulators at once.  Whole runs of MANY INDEPENDENT AGENTS in one launch, one
// wave per agent.  A translation unit of its own: no existing code object depends on it.
//
// Where the members live.  cacla_safe_kernel runs the simulator's sw::euler_step and the cost redundantly in all 64
// lanes of the agent's wave and takes the first lane's answer.  Here lane L holds the constants of member L % n_member
// -- derived in the kernel with sw::consts_of from the member's (l_i, m_i, k) and the real h and direction: the host's
// bits, and the bits cacla_safe_kernel gives that simulator -- so the same instructions look ahead in every member.
// The six member-dependent doubles of sw::Consts (l, kl_nm, h_kl_nm, six_k_m, kl_m, c12) are in VGPRs; h, dirx and diry
// stay uniform.  Every lane is active in the look-ahead, and with n_member < 64 members repeat: no lane is masked.
// MORE THAN 64 MEMBERS (a second wave per agent) IS NOT BUILT.
//
// One step of a gated agent: FA_act = actors(state), action = FA_act + noise[t] (consumed whether or not the step is
// taken); in every lane the look-ahead of its member from the same state with the same action and
// in = cost(sim_state) <= sim_thresh (NaN refuses; false in the lanes of a member that breaks the parameter rule, which
// look ahead with the real constants and not with the member's).  admit = every lane's `in`, through a wave ballot into
// scalar registers; the real step with the learner's update behind it is a uniform branch, as in cacla_safe_kernel.
// A refused step changes nothing.  Lane t & 63 keeps step t's reward entry, admit flag and worst cost; they are stored
// once per 64-step block.
//
// The two optional records.  worst_rec[t] = max over the lanes of (in-range cost, NaN or a bad member -> +inf): the map
// comes first, and a maximum of non-NaN doubles is exact in any order, so the reduction (four DPP steps inside a
// 16-lane row, then the four rows through scalar registers) needs no order contract.  It sits behind a uniform branch:
// a launch without worst_rec does not pay for it.  member_refusals[e]: lane e < n_member counts the steps at which
// its own `in` was false, one VALU add per step, and adds the count to memory at the end.
#include "swimmer_cacla_learner.h"

namespace {

constexpr int kEnsCaclaBlock = kWave;   // one wave per agent, one workgroup per wave

struct EnsCaclaArgs {
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
    return fmax(fmax(cacla::lane_value(v, 0), cacla::lane_value(v, 16)),
                fmax(cacla::lane_value(v, 32), cacla::lane_value(v, 48)));
}

template <int N>
__global__ void __launch_bounds__(kEnsCaclaBlock)
cacla_ensemble_kernel(sw::Consts C, int32_t n_member, int32_t n_iter, int32_t t_begin, int32_t cost_kind,
                      int32_t cost_index, EnsCaclaArgs a)
{
    using S = cacla::Shape<N>;
    constexpr int D = S::D, M = S::M, UPL = S::UPL;
    constexpr unsigned long long kEveryLane = ~0ull;
    __shared__ double prod[2][kWave * UPL];            // products of the forward at s (0) and at s' (1)

    const int lane = threadIdx.x;
    const int64_t agent = blockIdx.x;
    const cacla::Place pl = cacla::place_of<N>(lane);

    double *const wn = a.weights + (agent * N + pl.net) * S::NETD;
    double W1[UPL][D], b1[UPL], W2[UPL], b2;
    cacla::load_weights<N>(wn, pl.j0, W1, b1, W2, b2);

    double *const sp = a.state + agent * D;
    double gdx, gdy, th[N], thd[N];
    cacla::load_state<N>(sp, gdx, gdy, th, thd);
    const double gam = a.gamma[agent], alp = a.alpha[agent];

    // the gate: whether there is one (wave-uniform, like the thresholds), and THIS LANE's member
    const bool gated = __builtin_amdgcn_readfirstlane(a.gated[agent]) != 0;
    const double real_thresh = uniform_f64(a.real_thresh[agent]);
    double sim_thresh = 0.0;
    sw::Consts Cs = C;        // a bad member's lanes keep the real constants: its own are not used
    bool mem_ok = true;       // this lane's member satisfies the parameter rule
    bool sim_ok = true;       // every member does (uniform)
    if (gated) {   // uniform: an ungated agent reads neither sims nor sim_thresh
        const double *const sm = a.sims + (agent * n_member + lane % n_member) * 3;
        const double sim_l = sm[0], sim_m = sm[1], sim_k = sm[2];
        mem_ok = sim_params_ok(sim_l, sim_m, sim_k);
        if (mem_ok) Cs = sw::consts_of(N, sim_l, sim_m, sim_k, C.h, C.dirx, C.diry);
        sim_ok = __builtin_amdgcn_ballot_w64(mem_ok) == kEveryLane;
        sim_thresh = uniform_f64(a.sim_thresh[agent]);
    }

    const double *const np = a.noise + agent * (int64_t)n_iter * M;
    double nz[M], nz_next[M];
    cacla::load_noise<N>(np, n_iter, 0, lane, nz);

    double *const rp = a.rewards + agent * (int64_t)n_iter;
    int32_t *const ap = a.admitted_rec ? a.admitted_rec + agent * (int64_t)n_iter : nullptr;
    double *const wp = a.worst_rec ? a.worst_rec + agent * (int64_t)n_iter : nullptr;
    double last = uniform_f64(a.last_reward[agent]);     // the reward entry of a refused step
    double rstage = 0.0, wstage = 0.0;
    int32_t astage = 0;
    bool ok = true;
    double thmax = 0.0;
    int32_t n_upd = 0, n_adm = 0, n_viol = 0, refused_at = -1;
    int32_t n_out = 0;        // per lane: the steps at which this lane's member did not admit

    for (int32_t t0 = 0; t0 < n_iter; t0 += kWave) {
        cacla::load_noise<N>(np, n_iter, t0 + kWave, lane, nz_next);   // a block ahead: consumed 64 steps from here
        const int32_t steps = (n_iter - t0 < kWave) ? n_iter - t0 : kWave;
        for (int32_t k = 0; k < steps; ++k) {
            thmax = sw::track_angle_range<N>(thmax, th);
            double x[D], h[UPL], out[N], act[M];
            bool off[UPL];
            cacla::observe<N>(gdx, gdy, th, thd, x);
            cacla::forward<N>(prod[0], pl, W1, b1, W2, b2, x, h, off, out);
#pragma unroll
            for (int i = 0; i < M; ++i) act[i] = __dadd_rn(out[i], cacla::lane_value(nz[i], k));   // mean + noise

            bool admit = true;
            double worst = __builtin_nan("");   // an ungated agent's entry
            if (gated) {   // uniform: every member's look-ahead from the real state, each in its lanes
                double sgx = gdx, sgy = gdy, sth[N], sthd[N], srew;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    sth[i] = th[i];
                    sthd[i] = thd[i];
                }
                (void)sw::euler_step<N>(Cs, sgx, sgy, sth, sthd, act, srew);
                const double c = safe_cost<N>(cost_kind, cost_index, sgx, sgy, sth, sthd);
                const bool in = mem_ok && c <= sim_thresh;   // NaN refuses, and so does a bad member
                n_out += in ? 0 : 1;
                admit = __builtin_amdgcn_ballot_w64(in) == kEveryLane;   // every member admits: a scalar
                if (wp) worst = wave_max_f64((mem_ok && c == c) ? c : __builtin_inf());   // uniform
            }
            if (admit) {   // uniform
                double rew;
                ok = sw::euler_step<N>(C, gdx, gdy, th, thd, act, rew) && ok;
                n_adm += 1;
                n_viol += (safe_cost<N>(cost_kind, cost_index, gdx, gdy, th, thd) > real_thresh) ? 1 : 0;
                last = rew;
                cacla::learn<N>(prod[1], pl, W1, b1, W2, b2, gdx, gdy, th, thd, x, h, off, out, act, rew, gam, alp,
                                n_upd);
            } else {
                refused_at = (refused_at < 0) ? t0 + k : refused_at;
            }
            rstage = (lane == k) ? last : rstage;
            astage = (lane == k) ? (admit ? 1 : 0) : astage;
            wstage = (lane == k) ? worst : wstage;
        }
        if (lane < steps) {                              // one coalesced store each per block (the last one partial)
            rp[t0 + lane] = rstage;
            if (ap) ap[t0 + lane] = astage;
            if (wp) wp[t0 + lane] = wstage;
        }
#pragma unroll
        for (int i = 0; i < M; ++i) nz[i] = nz_next[i];
    }

    if (pl.valid) cacla::store_weights<N>(wn, pl.j0, W1, b1, W2, b2);
    if (gated && a.member_refusals && lane < n_member)   // lane e < n_member holds member e
        a.member_refusals[agent * n_member + lane] += n_out;
    if (lane == 0) {
        const bool fin = cacla::store_state<N>(sp, gdx, gdy, th, thd);
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

}  // namespace

int sw_cacla_safe_ensemble_run_f64(const sw_params *real, int64_t n_agent, int32_t n_member, int32_t n_iter,
                                   int64_t t_begin, const double *gamma, const double *alpha, const double *noise,
                                   const int32_t *gated, const double *sims, const double *sim_thresh,
                                   const double *real_thresh, int32_t cost_kind, int32_t cost_index, double *weights,
                                   double *state, double *last_reward, double *rewards, int32_t *admitted_rec,
                                   double *worst_rec, int32_t *member_refusals, int32_t *counters,
                                   int32_t *first_refused, int32_t *status, void *stream)
{
    int rc = check_params(real);
    if (rc) return rc;
    if (!gamma || !alpha || !noise || !gated || !sims || !sim_thresh || !real_thresh || !weights || !state ||
        !last_reward || !rewards || !counters || !first_refused)
        return SW_ERR_NULL;
    if (n_agent < 1 || n_agent > INT32_MAX || n_iter < 0) return SW_ERR_SIZE;   // grid.x: one workgroup per agent
    if (n_member < 1 || n_member > kWave) return SW_ERR_SIZE;                   // the members ride in one wave's lanes
    if (t_begin < 0 || t_begin > (int64_t)INT32_MAX - n_iter) return SW_ERR_SIZE;   // first_refused is an int32 step
    if (cost_kind != SW_COST_ABS_OBS && cost_kind != SW_COST_MAX_ABS_THETADOT) return SW_ERR_SIZE;
    if (cost_kind == SW_COST_ABS_OBS && (cost_index < 0 || cost_index >= 2 * real->n + 2)) return SW_ERR_SIZE;
    if (is_twin(real)) return SW_ERR_PARAM;
    if (n_iter == 0) return SW_OK;
    const sw::Consts C = make_consts(real);
    const EnsCaclaArgs a{gamma,   alpha,       noise,   gated,        sims,      sim_thresh,      real_thresh, weights,
                         state,   last_reward, rewards, admitted_rec, worst_rec, member_refusals, counters,
                         first_refused, status};
    const bool known_n = with_n<2, 8>(real->n, [&](auto N) {
        hipLaunchKernelGGL((cacla_ensemble_kernel<N.value>), dim3((unsigned)n_agent), dim3(kEnsCaclaBlock), 0,
                           (hipStream_t)stream, C, n_member, n_iter, (int32_t)t_begin, cost_kind, cost_index, a);
    });
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}
