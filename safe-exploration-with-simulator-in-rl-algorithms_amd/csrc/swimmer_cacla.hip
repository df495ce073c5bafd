// swimmer_cacla.hip -- CACLA on the swimmer (cacla/cacla_agent.py:135-199): whole training runs of MANY INDEPENDENT
// AGENTS in one launch, one wave per agent, n_iter strictly sequential steps each.  A translation unit of its own:
// it shares no shuffle helper with the families of swimmer_kernels.hip, so their machine code does not depend on it.
//
// The learner -- the layout of an agent's networks over its wave, the forward with its fixed summation order, the
// update, the noise a block ahead -- is swimmer_cacla_learner.h, whose header explains it.  This file's own: the
// TRAIN = false path, and the rewards: lane t & 63 keeps step t's reward, stored -- one coalesced vector store --
// every 64 steps and once more for the last partial block.
#include "swimmer_cacla_learner.h"

namespace {

constexpr int kCaclaBlock = kWave;       // one wave per agent, one workgroup per wave: a SIMD to itself

// TRAIN = false is the reference as written (cacla_agent.py:173-178): no updates and `state` never advanced -- the
// actors are evaluated at the observation the call started from at every step while the environment keeps stepping.
template <int N, bool TRAIN>
__global__ void __launch_bounds__(kCaclaBlock)
cacla_kernel(sw::Consts C, int32_t n_iter, const double *__restrict__ gamma, const double *__restrict__ alpha,
             const double *__restrict__ noise, double *__restrict__ weights, double *__restrict__ state,
             double *__restrict__ rewards, int32_t *__restrict__ actor_updates, int32_t *__restrict__ status)
{
    using S = cacla::Shape<N>;
    constexpr int D = S::D, M = S::M, UPL = S::UPL;
    __shared__ double prod[2][kWave * UPL];              // products of the forward at s (0) and at s' (1)

    const int lane = threadIdx.x;
    const int64_t agent = blockIdx.x;
    const cacla::Place pl = cacla::place_of<N>(lane);

    double *const wn = weights + (agent * N + pl.net) * S::NETD;
    double W1[UPL][D], b1[UPL], W2[UPL], b2;
    cacla::load_weights<N>(wn, pl.j0, W1, b1, W2, b2);

    double *const sp = state + agent * D;
    double gdx, gdy, th[N], thd[N];
    cacla::load_state<N>(sp, gdx, gdy, th, thd);
    double x0[D];                                        // TRAIN = false: the observation the actors keep seeing
    cacla::observe<N>(gdx, gdy, th, thd, x0);
    const double gam = gamma[agent], alp = alpha[agent];

    const double *const np = noise + agent * (int64_t)n_iter * M;
    double nz[M], nz_next[M];
    cacla::load_noise<N>(np, n_iter, 0, lane, nz);

    double *const rp = rewards + agent * (int64_t)n_iter;
    double rstage = 0.0;
    bool ok = true;
    double thmax = 0.0;
    int32_t n_upd = 0;

    for (int32_t t0 = 0; t0 < n_iter; t0 += kWave) {
        cacla::load_noise<N>(np, n_iter, t0 + kWave, lane, nz_next);   // a block ahead: consumed 64 steps from here
        const int32_t steps = (n_iter - t0 < kWave) ? n_iter - t0 : kWave;
        for (int32_t k = 0; k < steps; ++k) {
            thmax = sw::track_angle_range<N>(thmax, th);
            double x[D];
            if (TRAIN) {
                cacla::observe<N>(gdx, gdy, th, thd, x);
            } else {
#pragma unroll
                for (int i = 0; i < D; ++i) x[i] = x0[i];
            }
            double h[UPL], out[N], act[M];
            bool off[UPL];
            cacla::forward<N>(prod[0], pl, W1, b1, W2, b2, x, h, off, out);
#pragma unroll
            for (int i = 0; i < M; ++i) act[i] = __dadd_rn(out[i], cacla::lane_value(nz[i], k));   // mean + noise
            double rew;
            ok = sw::euler_step<N>(C, gdx, gdy, th, thd, act, rew) && ok;
            rstage = (lane == k) ? rew : rstage;
            if (TRAIN)
                cacla::learn<N>(prod[1], pl, W1, b1, W2, b2, gdx, gdy, th, thd, x, h, off, out, act, rew, gam, alp,
                                n_upd);
        }
        if (lane < steps) rp[t0 + lane] = rstage;        // one coalesced store per block (the last one partial)
#pragma unroll
        for (int i = 0; i < M; ++i) nz[i] = nz_next[i];
    }

    if (TRAIN && pl.valid) cacla::store_weights<N>(wn, pl.j0, W1, b1, W2, b2);
    if (lane == 0) {
        const bool fin = cacla::store_state<N>(sp, gdx, gdy, th, thd);
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
