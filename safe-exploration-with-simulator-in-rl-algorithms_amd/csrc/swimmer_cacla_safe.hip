// swimmer_cacla_safe.hip -- CACLA on the swimmer WITH SAFE EXPLORATION: the learner of swimmer_cacla_learner.h
// (cacla/cacla_agent.py:165-190; its header explains layout and summation order) inside the run loop of the reference's
// safe agents (cacla/cacla_safe_agent.py:161-188), every real step gated by a one-step look-ahead in the agent's
// simulator (safe_ars/ars.py:111-122).  Whole runs of MANY INDEPENDENT AGENTS in one launch, one wave per agent.  A
// translation unit of its own: no existing code object depends on it.
//
// An UNGATED agent (gated[a] == 0: no look-ahead, every step taken) runs the learner's pieces in cacla_kernel's order
// and so has the bits of sw_cacla_run_f64(train = 1).
//
// One step of a gated agent: FA_act = actors(state), action = FA_act + noise[t] (consumed whether or not the step is
// taken); the simulator's step from the same state with the same action (sw::euler_step with the agent's own
// constants, derived here with sw::consts_of: the host's bits); admitted = cost(sim_state) <= sim_thresh (NaN refuses).
// Every lane runs the look-ahead redundantly, so `admitted` is the same in all of them; it is taken from the first
// lane into a scalar register, and the real step with the learner's update behind it is a uniform branch.  A refused
// step changes nothing.  Lane t & 63 keeps step t's reward entry (the last admitted step's reward, NaN before the
// first admission) and its admit flag; both are stored once per 64-step block.
#include "swimmer_cacla_learner.h"

namespace {

constexpr int kSafeCaclaBlock = kWave;   // one wave per agent, one workgroup per wave

struct SafeCaclaArgs {
    const double *gamma, *alpha, *noise;
    const int32_t *gated;
    const double *sim, *sim_thresh, *real_thresh;
    double *weights, *state, *last_reward, *rewards;
    int32_t *admitted_rec, *counters, *first_refused, *status;
};

template <int N>
__global__ void __launch_bounds__(kSafeCaclaBlock)
cacla_safe_kernel(sw::Consts C, int32_t n_iter, int32_t t_begin, int32_t cost_kind, int32_t cost_index,
                  SafeCaclaArgs a)
{
    using S = cacla::Shape<N>;
    constexpr int D = S::D, M = S::M, UPL = S::UPL;
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

    // the gate: whether there is one, and the agent's simulator and thresholds (all wave-uniform)
    const bool gated = __builtin_amdgcn_readfirstlane(a.gated[agent]) != 0;
    const double real_thresh = uniform_f64(a.real_thresh[agent]);
    double sim_thresh = 0.0;
    sw::Consts Cs = C;
    bool sim_ok = true;
    if (gated) {   // uniform: an ungated agent reads neither sim nor sim_thresh
        const double sim_l = a.sim[agent * 3], sim_m = a.sim[agent * 3 + 1], sim_k = a.sim[agent * 3 + 2];
        sim_ok = __builtin_amdgcn_readfirstlane(sim_params_ok(sim_l, sim_m, sim_k) ? 1 : 0) != 0;
        if (sim_ok) Cs = uniform_consts(sw::consts_of(N, sim_l, sim_m, sim_k, C.h, C.dirx, C.diry));
        sim_thresh = uniform_f64(a.sim_thresh[agent]);
    }

    const double *const np = a.noise + agent * (int64_t)n_iter * M;
    double nz[M], nz_next[M];
    cacla::load_noise<N>(np, n_iter, 0, lane, nz);

    double *const rp = a.rewards + agent * (int64_t)n_iter;
    int32_t *const ap = a.admitted_rec ? a.admitted_rec + agent * (int64_t)n_iter : nullptr;
    double last = uniform_f64(a.last_reward[agent]);     // the reward entry of a refused step
    double rstage = 0.0;
    int32_t astage = 0;
    bool ok = true;
    double thmax = 0.0;
    int32_t n_upd = 0, n_adm = 0, n_viol = 0, refused_at = -1;

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
            if (gated) {   // uniform: the simulator's look-ahead from the real state (cacla_safe_agent.py:166-168)
                admit = false;
                if (sim_ok) {
                    double sgx = gdx, sgy = gdy, sth[N], sthd[N], srew;
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        sth[i] = th[i];
                        sthd[i] = thd[i];
                    }
                    (void)sw::euler_step<N>(Cs, sgx, sgy, sth, sthd, act, srew);
                    const bool in = safe_cost<N>(cost_kind, cost_index, sgx, sgy, sth, sthd) <= sim_thresh;   // NaN refuses
                    admit = __builtin_amdgcn_readfirstlane(in ? 1 : 0) != 0;   // every lane holds the same: lane 0's
                }
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
        }
        if (lane < steps) {                              // one coalesced store each per block (the last one partial)
            rp[t0 + lane] = rstage;
            if (ap) ap[t0 + lane] = astage;
        }
#pragma unroll
        for (int i = 0; i < M; ++i) nz[i] = nz_next[i];
    }

    if (pl.valid) cacla::store_weights<N>(wn, pl.j0, W1, b1, W2, b2);
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

int sw_cacla_safe_run_f64(const sw_params *real, int64_t n_agent, int32_t n_iter, int64_t t_begin,
                          const double *gamma, const double *alpha, const double *noise, const int32_t *gated,
                          const double *sim, const double *sim_thresh, const double *real_thresh, int32_t cost_kind,
                          int32_t cost_index, double *weights, double *state, double *last_reward, double *rewards,
                          int32_t *admitted_rec, int32_t *counters, int32_t *first_refused, int32_t *status,
                          void *stream)
{
    int rc = check_params(real);
    if (rc) return rc;
    if (!gamma || !alpha || !noise || !gated || !sim || !sim_thresh || !real_thresh || !weights || !state ||
        !last_reward || !rewards || !counters || !first_refused)
        return SW_ERR_NULL;
    if (n_agent < 1 || n_agent > INT32_MAX || n_iter < 0) return SW_ERR_SIZE;   // grid.x: one workgroup per agent
    if (t_begin < 0 || t_begin > (int64_t)INT32_MAX - n_iter) return SW_ERR_SIZE;   // first_refused is an int32 step
    if (cost_kind != SW_COST_ABS_OBS && cost_kind != SW_COST_MAX_ABS_THETADOT) return SW_ERR_SIZE;
    if (cost_kind == SW_COST_ABS_OBS && (cost_index < 0 || cost_index >= 2 * real->n + 2)) return SW_ERR_SIZE;
    if (is_twin(real)) return SW_ERR_PARAM;
    if (n_iter == 0) return SW_OK;
    const sw::Consts C = make_consts(real);
    const SafeCaclaArgs a{gamma,   alpha, noise,       gated,   sim,          sim_thresh, real_thresh,  weights,
                          state,   last_reward, rewards, admitted_rec, counters,   first_refused, status};
    const bool known_n = with_n<2, 8>(real->n, [&](auto N) {
        hipLaunchKernelGGL((cacla_safe_kernel<N.value>), dim3((unsigned)n_agent), dim3(kSafeCaclaBlock), 0,
                           (hipStream_t)stream, C, n_iter, (int32_t)t_begin, cost_kind, cost_index, a);
    });
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}
