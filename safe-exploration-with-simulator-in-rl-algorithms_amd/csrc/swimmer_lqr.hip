// swimmer_lqr.hip -- CACLA on small LQR problems, with and without safe exploration (cacla/cacla_agent.py:202-297,
// cacla/cacla_safe_agent.py, envs/gym_lqr/lqr_env.py): whole runs of MANY INDEPENDENT AGENTS in one launch, ONE AGENT
// PER LANE, n_iter strictly sequential steps each.  A translation unit of its own: it shares nothing with the kernel
// families of swimmer_kernels.hip, so their machine code does not depend on it.
//
// One step is the one written out in include/swimmer_hip.h (sw_lqr_cacla_run_f64): linear actor, Gaussian action,
// the simulator's step and the gate on its cost (safe runs), the real step, temporal difference, critic update and the
// conditional actor update.  An agent is a dozen to a hundred doubles, so everything it owns -- both models, Q, R,
// the hyper-parameters, F, V, the state, the last admitted record and the counters -- stays in this lane's VGPRs for
// the whole launch (the models differ between lanes: nothing of them can sit in SGPRs).  There is no cross-lane
// traffic, no LDS, no atomic; lanes behind the last agent leave at once.
//
// The chain is latency-bound, and memory is kept off it:
//  * every array is agent-minor ([..][agent]): a wave's access to one value of its 64 agents is one contiguous run;
//  * the noise does not depend on the state, so the kLqrAhead steps after the ones being computed are loaded while
//    those run (two register sets of kLqrAhead * NA doubles, swapped per block);
//  * records are plain vector stores that nothing waits for.
//
// Arithmetic follows the reference's order of operations where it writes one ((A s + B a) + C, (s' Q) s',
// (alpha td) s_j^2, (alpha (u_i - fa_i)) s_j); products may contract into FMAs.  Nothing is trapped: NaN and inf
// propagate, comparisons with NaN are false as in Python (a NaN cost is refused and counts as a violation of the real
// constraint, a NaN temporal difference updates no actor).
#include "swimmer_launch.h"

namespace {

constexpr int kLqrBlock = kWave;   // one wave per workgroup: 64 agents, spread over as many CUs as there are waves
constexpr int kLqrAhead = 8;       // steps per noise block: the loads of block b + 1 are issued before block b runs

// reset_inbound (lqr_env.py:80-93): M == 0 is no bound, otherwise |x| > M -> |x| / x * M.  |x| / x is +-1 for a
// finite x != 0 and NaN for +-inf (inf / inf) and for 0 (0 / 0: reachable only with M < 0); NaN > M is false.
__device__ __forceinline__ double lqr_clip(double x, double M)
{
    if (M != 0.0 && fabs(x) > M) {
        const double sign = (isinf(x) || x == 0.0) ? __builtin_nan("") : copysign(1.0, x);
        return sign * M;
    }
    return x;
}

// numpy.linalg.norm(x, inf | 2 | 1) of a vector: max |x_j| (a NaN wins, as numpy's max), sqrt(x . x), sum |x_j|
template <int NS>
__device__ __forceinline__ double lqr_cost(const double (&x)[NS], int32_t cost)
{
    // One coordinate: |x_0| whatever the norm (sqrt(x_0^2) where numpy takes it), as ONE select.  Written as the three
    // branches below, the inf- and the 1-norm are the same expression here, and the compiler's merge of the two left
    // the 1-norm's value undefined (the gate compared a stale register): tests/test_lqr_matrix_gpu.py, ns = 1,
    // SW_LQR_COST_1.  The branches are not instantiated for NS == 1.
    if constexpr (NS == 1) {
        const double a = fabs(x[0]);
        return cost == SW_LQR_COST_2 ? sqrt(x[0] * x[0]) : a;
    } else if (cost == SW_LQR_COST_INF) {
        double m = fabs(x[0]);
#pragma unroll
        for (int j = 1; j < NS; ++j) {
            const double a = fabs(x[j]);
            m = (a > m || a != a) ? a : m;
        }
        return m;
    } else if (cost == SW_LQR_COST_2) {
        double q = x[0] * x[0];
#pragma unroll
        for (int j = 1; j < NS; ++j) q += x[j] * x[j];
        return sqrt(q);
    } else {
        double q = fabs(x[0]);
#pragma unroll
        for (int j = 1; j < NS; ++j) q += fabs(x[j]);
        return q;
    }
}

template <int NS, int NA>
struct LqrModel {
    double A[NS][NS], B[NS][NA], C[NS], max_s, max_a;

    // row r of the SW_LQR_MODEL_DOUBLES block that starts at p[0] (agent stride `n`)
    __device__ __forceinline__ void load(const double *__restrict__ p, int64_t n)
    {
        int r = 0;
#pragma unroll
        for (int j = 0; j < NS; ++j)
#pragma unroll
            for (int k = 0; k < NS; ++k) A[j][k] = p[(r++) * n];
#pragma unroll
        for (int j = 0; j < NS; ++j)
#pragma unroll
            for (int i = 0; i < NA; ++i) B[j][i] = p[(r++) * n];
#pragma unroll
        for (int j = 0; j < NS; ++j) C[j] = p[(r++) * n];
        max_s = p[(r++) * n];
        max_a = p[(r++) * n];
    }

    // lqr_env.py:95-107 / :136-141: clip(A s + B clip(u) + C); `a` is the clipped action
    __device__ __forceinline__ void step(const double (&s)[NS], const double (&u)[NA], double (&a)[NA],
                                         double (&out)[NS]) const
    {
#pragma unroll
        for (int i = 0; i < NA; ++i) a[i] = lqr_clip(u[i], max_a);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            double as = A[j][0] * s[0];
#pragma unroll
            for (int k = 1; k < NS; ++k) as += A[j][k] * s[k];
            double ba = B[j][0] * a[0];
#pragma unroll
            for (int i = 1; i < NA; ++i) ba += B[j][i] * a[i];
            out[j] = lqr_clip((as + ba) + C[j], max_s);
        }
    }
};

// MODE 0: CACLA_LQR_agent.run; 1: safe, the simulator threshold of every step from its state and action
// (CACLA_LQR_SE_agent); 2: safe, the agent's fixed threshold (CACLA_LQR_SE_fix and its subclasses)
template <int NS, int NA, int MODE>
__global__ void __launch_bounds__(kLqrBlock)
lqr_cacla_kernel(int64_t n_agent, int32_t n_iter, int32_t cost, const double *__restrict__ params,
                 const double *__restrict__ noise, double *__restrict__ F_io, double *__restrict__ V_io,
                 double *__restrict__ state_io, double *__restrict__ last_io, int32_t *__restrict__ counters,
                 int32_t *__restrict__ status, double *__restrict__ rec_state, double *__restrict__ rec_action,
                 double *__restrict__ rec_reward, uint8_t *__restrict__ rec_admitted)
{
    constexpr bool SAFE = MODE != 0;
    constexpr int MD = SW_LQR_MODEL_DOUBLES(NS, NA);
    const int64_t agent = (int64_t)blockIdx.x * kLqrBlock + threadIdx.x;
    if (agent >= n_agent) return;            // no barrier, no cross-lane operation below
    const int64_t n = n_agent;

    LqrModel<NS, NA> real, sim;
    const double *const pp = params + agent;
    real.load(pp, n);
    if (SAFE) sim.load(pp + MD * n, n);
    double Q[NS][NS], R[NA][NA];
    {
        const double *q = pp + 2 * MD * n;
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) Q[i][j] = q[(i * NS + j) * n];
        q += NS * NS * n;
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int j = 0; j < NA; ++j) R[i][j] = q[(i * NA + j) * n];
    }
    const double *const hp = pp + (2 * MD + NS * NS + NA * NA) * n;
    const double gam = hp[0], alp = hp[n];
    const double lim = hp[2 * n], eps_lc = hp[3 * n], dA = hp[4 * n], dB = hp[5 * n], thr_fixed = hp[6 * n];

    double F[NA][NS], V[NS], s[NS];
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j) F[i][j] = F_io[(i * NS + j) * n + agent];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        V[j] = V_io[j * n + agent];
        s[j] = state_io[j * n + agent];
    }
    double last_s[NS], last_a[NA], last_r;   // the last admitted step's record (valid once n_adm > 0)
#pragma unroll
    for (int j = 0; j < NS; ++j) last_s[j] = last_io[j * n + agent];
#pragma unroll
    for (int i = 0; i < NA; ++i) last_a[i] = last_io[(NS + i) * n + agent];
    last_r = last_io[(NS + NA) * n + agent];
    int32_t n_adm = counters[agent], n_viol = counters[n + agent], n_upd = counters[2 * n + agent];

    const double *const nzp = noise + agent;
    auto load_noise = [&](int32_t t0, double (&dst)[kLqrAhead][NA]) {
#pragma unroll
        for (int k = 0; k < kLqrAhead; ++k) {
            const int64_t t = (int64_t)t0 + k;
#pragma unroll
            for (int i = 0; i < NA; ++i) dst[k][i] = (t < n_iter) ? nzp[(t * NA + i) * n] : 0.0;
        }
    };
    double nz[kLqrAhead][NA], nz_next[kLqrAhead][NA];
    load_noise(0, nz);

    for (int32_t t0 = 0; t0 < n_iter; t0 += kLqrAhead) {
        load_noise(t0 + kLqrAhead, nz_next);             // a block ahead: consumed kLqrAhead steps from here
#pragma unroll
        for (int k = 0; k < kLqrAhead; ++k) {
            const int64_t t = (int64_t)t0 + k;
            if (t >= n_iter) break;                      // wave-uniform
            double fa[NA], u[NA];
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                double f = F[i][0] * s[0];
#pragma unroll
                for (int j = 1; j < NS; ++j) f += F[i][j] * s[j];
                fa[i] = f;
                u[i] = f + nz[k][i];                     // Gaussian policy: mean + noise
            }
            bool admitted = true;
            if (SAFE) {
                double thr = thr_fixed;
                if (MODE == 1) {                         // compute_sim_threshold (cacla_safe_agent.py:63-73), u unclipped
                    double qs = s[0] * s[0], qu = u[0] * u[0];
#pragma unroll
                    for (int j = 1; j < NS; ++j) qs += s[j] * s[j];
#pragma unroll
                    for (int i = 1; i < NA; ++i) qu += u[i] * u[i];
                    thr = lim - eps_lc * (dA * sqrt(qs) + dB * sqrt(qu));
                }
                double a_sim[NA], s_sim[NS];
                sim.step(s, u, a_sim, s_sim);
                admitted = lqr_cost<NS>(s_sim, cost) <= thr;
            }
            if (admitted) {
                double a[NA], sn[NS];
                real.step(s, u, a, sn);
                double xq = 0.0, ar = 0.0;               // (s' Q) s' and (a R) a
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    double c = sn[0] * Q[0][j];
#pragma unroll
                    for (int i = 1; i < NS; ++i) c += sn[i] * Q[i][j];
                    xq = (j == 0) ? c * sn[0] : xq + c * sn[j];
                }
#pragma unroll
                for (int j = 0; j < NA; ++j) {
                    double c = a[0] * R[0][j];
#pragma unroll
                    for (int i = 1; i < NA; ++i) c += a[i] * R[i][j];
                    ar = (j == 0) ? c * a[0] : ar + c * a[j];
                }
                const double rew = -(xq + ar);
                if (SAFE) n_viol += (lqr_cost<NS>(sn, cost) <= lim) ? 0 : 1;   // the reference only prints
                double v_old = V[0] * (s[0] * s[0]), v_new = V[0] * (sn[0] * sn[0]);
#pragma unroll
                for (int j = 1; j < NS; ++j) {
                    v_old += V[j] * (s[j] * s[j]);
                    v_new += V[j] * (sn[j] * sn[j]);
                }
                const double td = (rew + gam * v_new) - v_old;
                const double cstep = alp * td;
#pragma unroll
                for (int j = 0; j < NS; ++j) V[j] += cstep * (s[j] * s[j]);
                if (td > 0.0) {                          // false for NaN
#pragma unroll
                    for (int i = 0; i < NA; ++i) {
                        const double astep = alp * (u[i] - fa[i]);
#pragma unroll
                        for (int j = 0; j < NS; ++j) F[i][j] += astep * s[j];
                    }
                    ++n_upd;
                }
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    last_s[j] = s[j];
                    s[j] = sn[j];
                }
#pragma unroll
                for (int i = 0; i < NA; ++i) last_a[i] = a[i];
                last_r = rew;
                ++n_adm;
            }
            if (rec_state) {
#pragma unroll
                for (int j = 0; j < NS; ++j) rec_state[(t * NS + j) * n + agent] = last_s[j];
            }
            if (rec_action) {
#pragma unroll
                for (int i = 0; i < NA; ++i) rec_action[(t * NA + i) * n + agent] = last_a[i];
            }
            if (rec_reward) rec_reward[t * n + agent] = last_r;
            if (rec_admitted)
                rec_admitted[t * n + agent] = admitted ? SW_LQR_ADMITTED : (n_adm > 0 ? SW_LQR_REFUSED : SW_LQR_NOTHING_YET);
        }
#pragma unroll
        for (int k = 0; k < kLqrAhead; ++k)
#pragma unroll
            for (int i = 0; i < NA; ++i) nz[k][i] = nz_next[k][i];
    }

    bool fin = true;
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            F_io[(i * NS + j) * n + agent] = F[i][j];
            fin = fin && isfinite(F[i][j]);
        }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        V_io[j * n + agent] = V[j];
        state_io[j * n + agent] = s[j];
        last_io[j * n + agent] = last_s[j];
        fin = fin && isfinite(V[j]) && isfinite(s[j]);
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) last_io[(NS + i) * n + agent] = last_a[i];
    last_io[(NS + NA) * n + agent] = last_r;
    counters[agent] = n_adm;
    counters[n + agent] = n_viol;
    counters[2 * n + agent] = n_upd;
    if (!fin) status[agent] |= SW_STATUS_NONFINITE;
}

}  // namespace

int sw_lqr_cacla_run_f64(int32_t ns, int32_t na, int64_t n_agent, int32_t n_iter, int32_t safe, int32_t threshold,
                         int32_t cost, const double *params, const double *noise, double *F, double *V, double *state,
                         double *last, int32_t *counters, int32_t *status, double *rec_state, double *rec_action,
                         double *rec_reward, uint8_t *rec_admitted, void *stream)
{
    (void)hipGetLastError();   // as check_params(): launch_status() below reports this call's launch only
    if (!params || !noise || !F || !V || !state || !last || !counters || !status) return SW_ERR_NULL;
    if (n_agent < 1 || n_agent > INT32_MAX || n_iter < 0) return SW_ERR_SIZE;
    if (ns < 1 || ns > SW_LQR_MAX_STATE || na < 1 || na > SW_LQR_MAX_ACTION) return SW_ERR_SIZE;
    if ((safe != 0 && safe != 1) || (threshold != SW_LQR_THRESHOLD_STEP && threshold != SW_LQR_THRESHOLD_FIXED) ||
        (cost != SW_LQR_COST_INF && cost != SW_LQR_COST_2 && cost != SW_LQR_COST_1))
        return SW_ERR_PARAM;
    if (n_iter == 0) return SW_OK;
    const int mode = !safe ? 0 : threshold == SW_LQR_THRESHOLD_STEP ? 1 : 2;
    const unsigned grid = (unsigned)((n_agent + kLqrBlock - 1) / kLqrBlock);
    with_n<1, SW_LQR_MAX_STATE>(ns, [&](auto NS) {
        with_n<1, SW_LQR_MAX_ACTION>(na, [&](auto NA) {
            with_n<0, 2>(mode, [&](auto MODE) {
                hipLaunchKernelGGL((lqr_cacla_kernel<NS.value, NA.value, MODE.value>), dim3(grid), dim3(kLqrBlock), 0,
                                   (hipStream_t)stream, n_agent, n_iter, cost, params, noise, F, V, state, last,
                                   counters, status, rec_state, rec_action, rec_reward, rec_admitted);
            });
        });
    });
    return launch_status();
}
