// swimmer_cacla_safe.hip -- CACLA on the swimmer WITH SAFE EXPLORATION: the learner of swimmer_cacla.hip
// (cacla/cacla_agent.py:165-190) inside the run loop of the reference's safe agents (cacla/cacla_safe_agent.py:161-188),
// every real step gated by a one-step look-ahead in the agent's simulator (safe_ars/ars.py:111-122).  Whole runs of
// MANY INDEPENDENT AGENTS in one launch, one wave per agent.  A translation unit of its own: no existing code object
// depends on it.
//
// The layout is cacla_kernel's (swimmer_cacla.hip, whose header explains it): the hidden units of an agent's n
// networks in the lanes of its wave, a unit's weights in registers for the whole run, every lane integrating the same
// swimmer, a network's output summed through LDS in the fixed order of sum_hidden() and handed out with v_readlane,
// the noise loaded a 64-step block ahead.  The learner's arithmetic -- forward, temp_diff, the two SGD steps -- is
// written expression by expression as it is there, so that an UNGATED agent (gated[a] == 0: no look-ahead, every step
// taken) has the bits of sw_cacla_run_f64(train = 1).
//
// One step of a gated agent: FA_act = actors(state), action = FA_act + noise[t] (consumed whether or not the step is
// taken); the simulator's step from the same state with the same action (sw::euler_step with the agent's own
// constants, derived here with sw::consts_of: the host's bits); admitted = cost(sim_state) <= sim_thresh (NaN refuses).
// Every lane runs the look-ahead redundantly, so `admitted` is the same in all of them; it is taken from the first
// lane into a scalar register, and the real step with the learner's update behind it is a uniform branch.  A refused
// step changes nothing.  Lane t & 63 keeps step t's reward entry (the last admitted step's reward, NaN before the
// first admission) and its admit flag; both are stored once per 64-step block.
#include "swimmer_launch.h"

namespace {

constexpr int kSafeCaclaBlock = kWave;   // one wave per agent, one workgroup per wave
constexpr int kHid = SW_CACLA_HIDDEN;

// v of lane `src` (wave-uniform) in every lane, through scalar registers.
__device__ __forceinline__ double lane_value(double v, int src)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// The order of a network's sum (swimmer_cacla.hip); __dadd_rn: no reassociation, no contraction.
__device__ __forceinline__ double sum_hidden(const double *q)
{
    const double a0 = __dadd_rn(q[0], q[1]), a1 = __dadd_rn(q[2], q[3]), a2 = __dadd_rn(q[4], q[5]);
    const double a3 = __dadd_rn(q[6], q[7]), a4 = __dadd_rn(q[8], q[9]), a5 = __dadd_rn(q[10], q[11]);
    return __dadd_rn(__dadd_rn(__dadd_rn(a0, a1), __dadd_rn(a2, a3)), __dadd_rn(a4, a5));
}

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
    constexpr int D = 2 * N + 2, M = N - 1;
    constexpr int UPL = (kHid * N <= kWave) ? 1 : 2;   // hidden units per lane
    constexpr int LPN = kHid / UPL;                    // lanes per network
    constexpr int NETD = SW_CACLA_NET_DOUBLES(N);
    static_assert(LPN * N <= kWave && kHid % UPL == 0, "an agent's networks must fit one wave");
    __shared__ double prod[2][kWave * UPL];            // products of the forward at s (0) and at s' (1)

    const int lane = threadIdx.x;
    const int64_t agent = blockIdx.x;
    const bool valid = lane < LPN * N;
    const int net = valid ? lane / LPN : N - 1;          // idle lanes shadow the critic's unit 0 and store nothing
    const int j0 = valid ? (lane % LPN) * UPL : 0;

    double *const wn = a.weights + (agent * N + net) * NETD;
    double W1[UPL][D], b1[UPL], W2[UPL], b2;
#pragma unroll
    for (int u = 0; u < UPL; ++u) {
#pragma unroll
        for (int i = 0; i < D; ++i) W1[u][i] = wn[(j0 + u) * D + i];
        b1[u] = wn[kHid * D + j0 + u];
        W2[u] = wn[kHid * D + kHid + j0 + u];
    }
    b2 = wn[kHid * D + 2 * kHid];

    double *const sp = a.state + agent * D;
    double gdx = sp[0], gdy = sp[1], th[N], thd[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        th[i] = sp[2 + 2 * i];
        thd[i] = sp[3 + 2 * i];
    }
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

    // this lane's step of a 64-step block: its n - 1 noise values
    const double *const np = a.noise + agent * (int64_t)n_iter * M;
    auto load_noise = [&](int32_t t0, double (&dst)[M]) {
        const int64_t t = (int64_t)t0 + lane;
#pragma unroll
        for (int i = 0; i < M; ++i) dst[i] = (t < n_iter) ? np[t * M + i] : 0.0;
    };
    double nz[M], nz_next[M];
    load_noise(0, nz);

    double *const rp = a.rewards + agent * (int64_t)n_iter;
    int32_t *const ap = a.admitted_rec ? a.admitted_rec + agent * (int64_t)n_iter : nullptr;
    double last = uniform_f64(a.last_reward[agent]);     // the reward entry of a refused step
    double rstage = 0.0;
    int32_t astage = 0;
    bool ok = true;
    double thmax = 0.0;
    int32_t n_upd = 0, n_adm = 0, n_viol = 0, refused_at = -1;

    for (int32_t t0 = 0; t0 < n_iter; t0 += kWave) {
        load_noise(t0 + kWave, nz_next);                 // a block ahead: consumed 64 steps from here
        const int32_t steps = (n_iter - t0 < kWave) ? n_iter - t0 : kWave;
        for (int32_t k = 0; k < steps; ++k) {
            thmax = sw::track_angle_range<N>(thmax, th);
            double x[D];
            x[0] = gdx;
            x[1] = gdy;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                x[2 + 2 * i] = th[i];
                x[3 + 2 * i] = thd[i];
            }
            // forward of every network at x.  relu as torch's: NaN passes (z <= 0 is false), and so does its gradient
            double h[UPL];
            bool off[UPL];
#pragma unroll
            for (int u = 0; u < UPL; ++u) {
                double z0 = b1[u], z1 = W1[u][1] * x[1];
                z0 = __builtin_fma(W1[u][0], x[0], z0);
#pragma unroll
                for (int i = 2; i < D; i += 2) {
                    z0 = __builtin_fma(W1[u][i], x[i], z0);
                    z1 = __builtin_fma(W1[u][i + 1], x[i + 1], z1);
                }
                const double z = z0 + z1;
                off[u] = z <= 0.0;
                h[u] = off[u] ? 0.0 : z;
                prod[0][lane * UPL + u] = W2[u] * h[u];
            }
            __syncthreads();
            const double own = __dadd_rn(sum_hidden(&prod[0][net * kHid]), b2);
            double out[N];                               // actors' outputs, then V(x): wave-uniform
#pragma unroll
            for (int i = 0; i < N; ++i) out[i] = lane_value(own, i * LPN);

            double act[M];                               // Gaussian policy: mean + noise
#pragma unroll
            for (int i = 0; i < M; ++i) act[i] = __dadd_rn(out[i], lane_value(nz[i], k));

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
                // V(s') with the weights from before this step's update (cacla_agent.py:186)
#pragma unroll
                for (int u = 0; u < UPL; ++u) {
                    double z0 = b1[u], z1 = W1[u][1] * gdy;
                    z0 = __builtin_fma(W1[u][0], gdx, z0);
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        z0 = __builtin_fma(W1[u][2 + 2 * i], th[i], z0);
                        z1 = __builtin_fma(W1[u][3 + 2 * i], thd[i], z1);
                    }
                    const double z = z0 + z1;
                    prod[1][lane * UPL + u] = W2[u] * ((z <= 0.0) ? 0.0 : z);
                }
                __syncthreads();
                const double v_new = lane_value(__dadd_rn(sum_hidden(&prod[1][net * kHid]), b2), (N - 1) * LPN);
                const double td = __dadd_rn(__dadd_rn(rew, __dmul_rn(gam, v_new)), -out[N - 1]);
                const bool better = td > 0.0;            // false for NaN: no actor update, as the reference
                n_upd += better ? 1 : 0;
                // this lane's network: the critic steps by alpha td, actor i by alpha (action_i - FA_act_i) if better
                double st = __dmul_rn(alp, td);
                bool upd = true;
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    const double sa = __dmul_rn(alp, __dadd_rn(act[i], -out[i]));
                    st = (net == i) ? sa : st;
                    upd = (net == i) ? better : upd;
                }
                if (upd) {
#pragma unroll
                    for (int u = 0; u < UPL; ++u) {
                        const double sg = st * (off[u] ? 0.0 : W2[u]);   // the OLD W2
                        W2[u] = __builtin_fma(st, h[u], W2[u]);
#pragma unroll
                        for (int i = 0; i < D; ++i) W1[u][i] = __builtin_fma(sg, x[i], W1[u][i]);
                        b1[u] += sg;
                    }
                    b2 += st;
                }
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

    if (valid) {
#pragma unroll
        for (int u = 0; u < UPL; ++u) {
#pragma unroll
            for (int i = 0; i < D; ++i) wn[(j0 + u) * D + i] = W1[u][i];
            wn[kHid * D + j0 + u] = b1[u];
            wn[kHid * D + kHid + j0 + u] = W2[u];
        }
        if (j0 == 0) wn[kHid * D + 2 * kHid] = b2;
    }
    if (lane == 0) {
        sp[0] = gdx;
        sp[1] = gdy;
        bool fin = isfinite(gdx) && isfinite(gdy);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            sp[2 + 2 * i] = th[i];
            sp[3 + 2 * i] = thd[i];
            fin = fin && isfinite(th[i]) && isfinite(thd[i]);
        }
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
