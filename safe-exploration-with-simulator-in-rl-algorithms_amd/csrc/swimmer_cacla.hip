// swimmer_cacla.hip -- CACLA on the swimmer (cacla/cacla_agent.py:135-199): whole training runs of MANY INDEPENDENT
// AGENTS in one launch, one wave per agent, n_iter strictly sequential steps each.  A translation unit of its own:
// it shares no shuffle helper with the families of swimmer_kernels.hip, so their machine code does not depend on it.
//
// One step (cacla_agent.py:170-193): actor forward, Gaussian action, physics step, critic at the new and at the old
// state, SGD step on the critic, SGD step on the actors when the temporal difference is positive.  No clipping, no
// reset, `done` ignored -- as the reference.
//
// Where things live.  An agent has n networks -- n - 1 actors (one per torque, ActorFA) and the critic (CriticFA), in
// that order -- each TwoLayersNet(d = 2n + 2, 12) in fp64.  Their 12 n hidden units are spread over the lanes of the
// agent's wave: unit j of network k sits in lane 12 k + j (n <= 5: one unit per lane), or units 2i, 2i + 1 of network
// k in lane 6 k + i (n >= 6: two per lane, 12 n > 64).  A unit's lane keeps W1[j, :], b1[j] and W2[j] in registers
// for the whole run; every lane of a network keeps a copy of its b2 (all copies take the same updates).  The backward
// pass of update_weights is lane-local: with z_j, h_j from the forward at the same state and the weights unchanged
// since, g_j = relu'(z_j) W2_j (the OLD W2_j), W2_j += step h_j, b2 += step, W1[j, :] += step g_j x, b1_j += step
// g_j -- no second forward.  Every lane integrates the SAME swimmer (sw::euler_step<N>, redundantly: a wave's SIMD
// time does not depend on how many lanes do useful work), so every lane has the observation without a broadcast.
//
// The only cross-lane work is a network's output sum_j W2_j h_j + b2: n sums at the old state (the actors' and V(s))
// and V(s') -- n + 1 per step.  SUMMATION ORDER (fixed): the lanes write their products p_j to LDS; every lane of
// network k reads p_0 .. p_11 of ITS network (same addresses within a network: broadcast reads) and adds
//     ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), that + ((p8 + p9) + (p10 + p11)), that + b2;
// the value every lane then USES for network k is the one computed by the lane of k's unit 0, fetched with
// v_readlane into scalar registers.  Each sum is therefore computed in one place and is wave-uniform by
// construction: `temp_diff > 0`, the actions and the physics cannot differ between lanes.
//
// Memory traffic is off the critical path: lane l loads the noise of step 64 b + l of block b one block ahead
// (the n - 1 doubles of a step are contiguous, a block is one contiguous run), and step t takes its noise from lane
// t & 63 with v_readlane; lane t & 63 keeps step t's reward, stored -- one coalesced vector store -- every 64 steps
// and once more for the last partial block.
#include "swimmer_launch.h"

namespace {

constexpr int kCaclaBlock = kWave;       // one wave per agent, one workgroup per wave: a SIMD to itself
constexpr int kHid = SW_CACLA_HIDDEN;

// v of lane `src` (wave-uniform) in every lane, through scalar registers.
__device__ __forceinline__ double lane_value(double v, int src)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// The documented order of a network's sum (file header); __dadd_rn: no reassociation, no contraction.
__device__ __forceinline__ double sum_hidden(const double *q)
{
    const double a0 = __dadd_rn(q[0], q[1]), a1 = __dadd_rn(q[2], q[3]), a2 = __dadd_rn(q[4], q[5]);
    const double a3 = __dadd_rn(q[6], q[7]), a4 = __dadd_rn(q[8], q[9]), a5 = __dadd_rn(q[10], q[11]);
    return __dadd_rn(__dadd_rn(__dadd_rn(a0, a1), __dadd_rn(a2, a3)), __dadd_rn(a4, a5));
}

// TRAIN = false is the reference as written (cacla_agent.py:173-178): no updates and `state` never advanced -- the
// actors are evaluated at the observation the call started from at every step while the environment keeps stepping.
template <int N, bool TRAIN>
__global__ void __launch_bounds__(kCaclaBlock)
cacla_kernel(sw::Consts C, int32_t n_iter, const double *__restrict__ gamma, const double *__restrict__ alpha,
             const double *__restrict__ noise, double *__restrict__ weights, double *__restrict__ state,
             double *__restrict__ rewards, int32_t *__restrict__ actor_updates, int32_t *__restrict__ status)
{
    constexpr int D = 2 * N + 2, M = N - 1;
    constexpr int UPL = (kHid * N <= kWave) ? 1 : 2;   // hidden units per lane
    constexpr int LPN = kHid / UPL;                    // lanes per network
    constexpr int NETD = SW_CACLA_NET_DOUBLES(N);
    static_assert(LPN * N <= kWave && kHid % UPL == 0, "an agent's networks must fit one wave");
    // products of the forward at s (0) and at s' (1); lanes behind the last network write their own, unread slots
    __shared__ double prod[2][kWave * UPL];

    const int lane = threadIdx.x;
    const int64_t agent = blockIdx.x;
    const bool valid = lane < LPN * N;
    const int net = valid ? lane / LPN : N - 1;          // idle lanes shadow the critic's unit 0 and store nothing
    const int j0 = valid ? (lane % LPN) * UPL : 0;

    double *const wn = weights + (agent * N + net) * NETD;
    double W1[UPL][D], b1[UPL], W2[UPL], b2;
#pragma unroll
    for (int u = 0; u < UPL; ++u) {
#pragma unroll
        for (int i = 0; i < D; ++i) W1[u][i] = wn[(j0 + u) * D + i];
        b1[u] = wn[kHid * D + j0 + u];
        W2[u] = wn[kHid * D + kHid + j0 + u];
    }
    b2 = wn[kHid * D + 2 * kHid];

    double *const sp = state + agent * D;
    double gdx = sp[0], gdy = sp[1], th[N], thd[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        th[i] = sp[2 + 2 * i];
        thd[i] = sp[3 + 2 * i];
    }
    double x0[D];                                        // TRAIN = false: the observation the actors keep seeing
    x0[0] = gdx;
    x0[1] = gdy;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        x0[2 + 2 * i] = th[i];
        x0[3 + 2 * i] = thd[i];
    }
    const double gam = gamma[agent], alp = alpha[agent];

    // this lane's step of a 64-step block: its n - 1 noise values
    const double *const np = noise + agent * (int64_t)n_iter * M;
    auto load_noise = [&](int32_t t0, double (&dst)[M]) {
        const int64_t t = (int64_t)t0 + lane;
#pragma unroll
        for (int i = 0; i < M; ++i) dst[i] = (t < n_iter) ? np[t * M + i] : 0.0;
    };
    double nz[M], nz_next[M];
    load_noise(0, nz);

    double *const rp = rewards + agent * (int64_t)n_iter;
    double rstage = 0.0;
    bool ok = true;
    double thmax = 0.0;
    int32_t n_upd = 0;

    for (int32_t t0 = 0; t0 < n_iter; t0 += kWave) {
        load_noise(t0 + kWave, nz_next);                 // a block ahead: consumed 64 steps from here
        const int32_t steps = (n_iter - t0 < kWave) ? n_iter - t0 : kWave;
        for (int32_t k = 0; k < steps; ++k) {
            thmax = sw::track_angle_range<N>(thmax, th);
            double x[D];
            if (TRAIN) {
                x[0] = gdx;
                x[1] = gdy;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    x[2 + 2 * i] = th[i];
                    x[3 + 2 * i] = thd[i];
                }
            } else {
#pragma unroll
                for (int i = 0; i < D; ++i) x[i] = x0[i];
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

            double act[M];                               // Gaussian policy: mean + noise (cacla_agent.py:182)
#pragma unroll
            for (int i = 0; i < M; ++i) act[i] = __dadd_rn(out[i], lane_value(nz[i], k));
            double rew;
            ok = sw::euler_step<N>(C, gdx, gdy, th, thd, act, rew) && ok;
            rstage = (lane == k) ? rew : rstage;

            if (TRAIN) {
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
            }
        }
        if (lane < steps) rp[t0 + lane] = rstage;        // one coalesced store per block (the last one partial)
#pragma unroll
        for (int i = 0; i < M; ++i) nz[i] = nz_next[i];
    }

    if (TRAIN && valid) {
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
        if (status)
            status[agent] |= (ok ? 0 : SW_STATUS_SINGULAR) | (fin ? 0 : SW_STATUS_NONFINITE) |
                             (thmax < sw::kAngleLimit ? 0 : SW_STATUS_RANGE);
        if (actor_updates) actor_updates[agent] += n_upd;
    }
}

}  // namespace

int sw_cacla_run_f64(const sw_params *p, int64_t n_agent, int32_t n_iter, int32_t train, const double *gamma,
                     const double *alpha, const double *noise, double *weights, double *state, double *rewards,
                     int32_t *actor_updates, int32_t *status, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (!gamma || !alpha || !noise || !weights || !state || !rewards) return SW_ERR_NULL;
    if (n_agent < 1 || n_agent > INT32_MAX || n_iter < 0) return SW_ERR_SIZE;   // grid.x: one workgroup per agent
    if (is_twin(p)) return SW_ERR_PARAM;
    if (n_iter == 0) return SW_OK;
    const sw::Consts C = make_consts(p);
    const bool known_n = with_n<2, 8>(p->n, [&](auto N, auto TRAIN) {
        hipLaunchKernelGGL((cacla_kernel<N.value, TRAIN.value>), dim3((unsigned)n_agent), dim3(kCaclaBlock), 0,
                           (hipStream_t)stream, C, n_iter, gamma, alpha, noise, weights, state, rewards,
                           actor_updates, status);
    }, train != 0);
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}
