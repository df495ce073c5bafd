// swimmer_rlglue_ars.hip -- the reference's RL-Glue experiment (rlglue/agent/SwimmerAgent.py driven by
// rlglue/experiment/SwimmerExperiment.cpp:65-84 on rlglue/environment/SwimmerEnvironment.cpp): whole ARS training runs
// of MANY INDEPENDENT AGENTS in one launch, ONE AGENT PER LANE, on the native (twin) swimmer model.  A translation unit
// of its own: it shares nothing with the kernel families of swimmer_kernels.hip, so their machine code does not depend
// on it.
//
// The agent is a step-counting state machine whose quirks chain every rollout ("segment": H environment steps from the
// saved start state) to the one before it; include/swimmer_hip.h (sw_rlglue_ars_run_f64) writes the loop out.  What
// matters here: the (2N + 1) H steps of an iteration are one serial chain per agent, so the launch is latency-bound
// and an agent's only parallelism is the other agents.  One wave per workgroup: waves spread over the CUs.
//
// What an agent owns, and where it lives:
//  * the state, the stale action, the running return: VGPRs for the whole launch;
//  * the segment's policy P +- nu delta (m d doubles, formed ONCE per segment): VGPRs for n <= kRegMaxN, otherwise this
//    lane's column of an LDS tile [m d][64] (conflict-free ds_read_b64, no barrier: a lane reads what it wrote).  126
//    doubles (n = 8) are 252 VGPRs next to a twin step whose own working set (the n x n system, cos and sin of every
//    angle difference: 3 n^2 doubles) is 384 VGPRs at n = 8;
//  * the agent's policy P, the deltas and the returns of the iteration: global memory, agent-minor, touched once per
//    segment (P, delta) resp. once per iteration (the update reads its own train_returns back) -- off the step loop.
//
// Arithmetic: the mat-vec is two partial sums in a fixed order, the return a plain running sum, the policy
// perturbation and the update are numpy's separate roundings (__dmul_rn / __dadd_rn / one division), sigma a two-pass
// sample standard deviation.  The clip is the agent's two comparisons (a NaN passes through).  Nothing is trapped.
#include "swimmer_launch.h"

namespace {

constexpr int kGlueBlock = kWave;   // one wave per workgroup: 64 agents
constexpr int kRegMaxN = 4;         // segment policy in VGPRs up to here (30 doubles), in LDS beyond

// SwimmerAgent.py:192-196
__device__ __forceinline__ double glue_clip(double a, double max_u)
{
    if (a > max_u)
        a = max_u;
    else if (a < -max_u)
        a = -max_u;
    return a;
}

// The policy of the running segment: entry k = i d + j of this lane's agent.
template <int K, bool IN_LDS>
struct SegPolicy;
template <int K>
struct SegPolicy<K, false> {
    double w[K];
    __device__ __forceinline__ explicit SegPolicy(double *) {}
    __device__ __forceinline__ double get(int k) const { return w[k]; }
    __device__ __forceinline__ void set(int k, double v) { w[k] = v; }
};
template <int K>
struct SegPolicy<K, true> {
    double *col;   // lds + lane
    __device__ __forceinline__ explicit SegPolicy(double *tile) : col(tile + threadIdx.x) {}
    __device__ __forceinline__ double get(int k) const { return col[k * kGlueBlock]; }
    __device__ __forceinline__ void set(int k, double v) { col[k * kGlueBlock] = v; }
};

// a = clip(W sm): two partial sums per row, even and odd columns (D is even)
template <int N, class W>
__device__ __forceinline__ void glue_action(const W &w, const double (&sm)[2 * N + 2], double max_u,
                                            double (&a)[N - 1])
{
    constexpr int D = 2 * N + 2, M = N - 1;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        double a0 = w.get(i * D) * sm[0], a1 = w.get(i * D + 1) * sm[1];
#pragma unroll
        for (int j = 2; j < D; j += 2) {
            a0 = __builtin_fma(w.get(i * D + j), sm[j], a0);
            a1 = __builtin_fma(w.get(i * D + j + 1), sm[j + 1], a1);
        }
        a[i] = glue_clip(a0 + a1, max_u);
    }
}

template <int N, bool IN_LDS>
__global__ void __launch_bounds__(kGlueBlock)
rlglue_ars_kernel(sw::TwinConsts T, double max_u, int64_t n_agent, int32_t fresh, int32_t n_iter, int32_t n_dir,
                  int32_t b, int32_t H, const double *__restrict__ alpha, const double *__restrict__ nu,
                  const double *__restrict__ deltas, double *policy, double *carry, double *eval_returns,
                  double *train_returns, int32_t *status)
{
    constexpr int D = 2 * N + 2, M = N - 1, K = M * D;
    __shared__ double tile[IN_LDS ? K * kGlueBlock : 1];
    const int64_t agent = (int64_t)blockIdx.x * kGlueBlock + threadIdx.x;
    if (agent >= n_agent) return;            // no barrier, no cross-lane operation below
    const int64_t n = n_agent;
    const int32_t n_seg = 2 * n_dir;         // exploration segments per iteration; segment n_seg is the evaluation

    const double alp = alpha[agent], nuu = nu[agent];
    double *const P = policy + agent;        // entry k at P[k n]
    SegPolicy<K, IN_LDS> w(tile);

    double s0[D];
#pragma unroll
    for (int j = 0; j < D; ++j) s0[j] = kTwinStart;

    double stale[M], total;
    if (fresh) {                             // agent_start (SwimmerAgent.py:61-77): pol(0) on the first observation
        const double *dl = deltas + agent;
#pragma unroll
        for (int k = 0; k < K; ++k) w.set(k, __dadd_rn(P[k * n], __dmul_rn(nuu, dl[k * n])));
        glue_action<N>(w, s0, max_u, stale);
        total = 0.0;
    } else {
#pragma unroll
        for (int i = 0; i < M; ++i) stale[i] = carry[i * n + agent];
        total = carry[M * n + agent];
    }

    bool ok = true, fin = true;
    double thmax = 0.0;                      // largest |theta| fed to sincos_fast
    for (int32_t it = 0; it < n_iter; ++it) {
        const double *const dit = deltas + (int64_t)it * n_dir * K * n + agent;   // direction i, entry k: dit[(i K + k) n]
        double *const rew = train_returns + (int64_t)it * n_seg * n + agent;      // entry j: rew[j n]
        for (int32_t j = 0; j <= n_seg; ++j) {
            const bool eval = j == n_seg;
            if (eval) {
                // update_policy (SwimmerAgent.py:223-239): sigma over rew[0 .. 2b), directions in index order
                const int32_t cnt = 2 * b;
                double sum = 0.0;
                for (int32_t i = 0; i < cnt; ++i) sum += rew[i * n];
                const double mean = sum / (double)cnt;
                double ss = 0.0;
                for (int32_t i = 0; i < cnt; ++i) {
                    const double e = rew[i * n] - mean;
                    ss = __builtin_fma(e, e, ss);
                }
                const double sigma = sqrt(ss / (double)(cnt - 1));
                const double den = __dmul_rn((double)b, sigma);
                for (int k = 0; k < K; ++k) {
                    double g = 0.0;
                    for (int32_t i = 0; i < b; ++i) {
                        const double diff = __dsub_rn(rew[(2 * i) * n], rew[(2 * i + 1) * n]);
                        g = __dadd_rn(g, __dmul_rn(diff, dit[((int64_t)i * K + k) * n]));
                    }
                    const double pk = __dadd_rn(P[k * n], __dmul_rn(alp, g / den));
                    P[k * n] = pk;
                    fin = fin && isfinite(pk);
                }
#pragma unroll
                for (int k = 0; k < K; ++k) w.set(k, P[k * n]);          // the frozen evaluation runs the new policy
            } else {
                const double sg = (j & 1) ? -nuu : nuu;                  // P - nu delta == P + (-nu) delta, bit for bit
                const double *const dl = dit + (int64_t)(j >> 1) * K * n;
#pragma unroll
                for (int k = 0; k < K; ++k) w.set(k, __dadd_rn(P[k * n], __dmul_rn(sg, dl[k * n])));
            }

            // one segment: H steps from the saved state ("load state", SwimmerExperiment.cpp:68-72).  Its first step
            // applies the action the agent chose at the END of the segment before, and the agent answers that step
            // with the INITIAL observation (SwimmerAgent.py:88-96, :100-104)
            double gdx = kTwinStart, gdy = kTwinStart, th[N], thd[N];
#pragma unroll
            for (int i = 0; i < N; ++i) th[i] = thd[i] = kTwinStart;
            double first = 0.0, rest = 0.0;
            for (int32_t t = 0; t < H; ++t) {            // ONE copy of the step: t == 0 differs by two selects
                thmax = sw::track_angle_range<N>(thmax, th);
                double r;
                ok = sw::twin_step<N>(T, gdx, gdy, th, thd, stale, r) && ok;
                const bool head = t == 0;                // wave-uniform
                first = head ? r : first;
                rest = head ? 0.0 : rest + r;
                double sm[D];
                sm[0] = head ? kTwinStart : gdx;
                sm[1] = head ? kTwinStart : gdy;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    sm[2 + 2 * i] = head ? kTwinStart : th[i];
                    sm[3 + 2 * i] = head ? kTwinStart : thd[i];
                }
                glue_action<N>(w, sm, max_u, stale);
            }
            fin = fin && isfinite(gdx) && isfinite(gdy);
#pragma unroll
            for (int i = 0; i < N; ++i) fin = fin && isfinite(th[i]) && isfinite(thd[i]);

            if (eval) {
                eval_returns[(int64_t)it * n + agent] = rest;            // "get total_reward" after the frozen rollout
                fin = fin && isfinite(rest);
            } else {
                // returns are credited one segment late (SwimmerAgent.py:89-93): segment 0 closes entry 2N - 1 with
                // what the evaluation before it left in `total`
                const double credited = total + first;
                rew[(int64_t)(j == 0 ? n_seg - 1 : j - 1) * n] = credited;
                fin = fin && isfinite(credited);
            }
            total = rest;
        }
    }

#pragma unroll
    for (int i = 0; i < M; ++i) carry[i * n + agent] = stale[i];
    carry[M * n + agent] = total;
    const int32_t code = (ok ? 0 : SW_STATUS_SINGULAR) | (fin ? 0 : SW_STATUS_NONFINITE) |
                         (thmax < sw::kAngleLimit ? 0 : SW_STATUS_RANGE);
    if (code) status[agent] |= code;
}

}  // namespace

int sw_rlglue_ars_run_f64(const sw_params *p, double max_u, int64_t n_agent, int64_t iter_begin, int32_t n_iter,
                          int32_t N, int32_t b, int32_t H, const double *alpha, const double *nu, const double *deltas,
                          double *policy, double *carry, double *eval_returns, double *train_returns, int32_t *status,
                          void *stream)
{
    (void)hipGetLastError();   // as check_params(): launch_status() below reports this call's launch only
    if (!p || !alpha || !nu || !deltas || !policy || !carry || !eval_returns || !train_returns || !status)
        return SW_ERR_NULL;
    if (n_agent < 1 || n_agent > INT32_MAX || n_iter < 0 || iter_begin < 0 || N < 1 || b < 1 || b > N || H < 1 ||
        N > INT32_MAX / 2)
        return SW_ERR_SIZE;
    const int rc = validate_params(p);
    if (rc) return rc;
    if (!is_twin(p) || !(max_u >= 0.0)) return SW_ERR_PARAM;   // NaN fails the comparison; +inf is "no clip"
    if (n_iter == 0) return SW_OK;
    const sw::TwinConsts T = make_twin_consts(p);
    const unsigned grid = (unsigned)((n_agent + kGlueBlock - 1) / kGlueBlock);
    const bool known_n = with_n<2, 8>(p->n, [&](auto NN) {
        hipLaunchKernelGGL((rlglue_ars_kernel<NN.value, (NN.value > kRegMaxN)>), dim3(grid), dim3(kGlueBlock), 0,
                           (hipStream_t)stream, T, max_u, n_agent, (int32_t)(iter_begin == 0), n_iter, N, b, H, alpha,
                           nu, deltas, policy, carry, eval_returns, train_returns, status);
    });
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}
