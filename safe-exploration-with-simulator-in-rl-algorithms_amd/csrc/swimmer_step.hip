// swimmer_step.hip -- one physics step for a batch of environments: step / accelerations / reset, the estimator's
// residual kernels (one parameter set, a population, or populations over many transition sets), the batch-1 environment (sw_env1), and their entry points.
//
// The kernels are put together from ONE copy of each piece, __device__ __forceinline__ function templates over arrays
// that stay plain locals of the kernels (a struct that owns the arrays costs registers, DESIGN.md "One learner, two
// kernels"): load_state / load_action / store_state and load_transition (the SoA columns), step_checked and
// accel_checked (the step and the accelerations with their NaN rules), residual_sq (the distance to the stored next
// state), wave_sum / post_wave_sum / waves_in_order / row_sum (the fixed-order sums), candidate_setup and
// score_candidates (a candidate's consts and the candidate loop).  What the tests promise bit for bit -- population
// and sets against the single kernel, env1 against the batched kernels, the row sums' order -- holds because these
// are the same functions, not because copies are kept in step.
#include <cstring>
#include <initializer_list>
#include <new>

#include "swimmer_launch.h"

namespace {

// ------------------------------------------------------------------------------------
// TWIN selects the reference's native model (swimmer_twin.h) instead of the Gym model.
// NT = nontemporal loads and stores: for batches that stream through HBM (larger than the
// 256 MiB Infinity Cache) they measured +6..8 % (16.8 M envs: 5.91 -> 6.37 TB/s); smaller
// batches keep plain accesses so that a step loop stays cache resident.
template <bool NT> __device__ __forceinline__ double ld_f64(const double *p)
{
    return NT ? __builtin_nontemporal_load(p) : *p;
}
template <bool NT> __device__ __forceinline__ void st_f64(double v, double *p)
{
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// Column e of a state array [2 + 2 N][n_env]: Gdot, then theta_i, thetadot_i.  The column's pointer is formed first
// and the rows are steps of n_env from it: with the row's offset multiplied out per element the plain kernels get
// 64-bit multiply-adds for what are chained adds here.
template <int N, bool NT>
__device__ __forceinline__ void load_state(const double *__restrict__ s, int64_t n_env, int64_t e, double &gdx,
                                           double &gdy, double (&th)[N], double (&thd)[N])
{
    const double *col = s + e;
    gdx = ld_f64<NT>(col);
    gdy = ld_f64<NT>(col + n_env);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        th[i] = ld_f64<NT>(col + (int64_t)(2 + 2 * i) * n_env);
        thd[i] = ld_f64<NT>(col + (int64_t)(3 + 2 * i) * n_env);
    }
}

template <int N, bool NT>
__device__ __forceinline__ void load_action(const double *__restrict__ act, int64_t n_env, int64_t e,
                                            double (&u)[N - 1])
{
    const double *col = act + e;
#pragma unroll
    for (int i = 0; i < N - 1; ++i) u[i] = ld_f64<NT>(col + (int64_t)i * n_env);
}

// Stores the column and returns SW_STATUS_NONFINITE unless every entry of it is finite (else 0).
template <int N, bool NT>
__device__ __forceinline__ int32_t store_state(double *__restrict__ s, int64_t n_env, int64_t e, double gdx, double gdy,
                                               const double (&th)[N], const double (&thd)[N])
{
    double *col = s + e;
    st_f64<NT>(gdx, col);
    st_f64<NT>(gdy, col + n_env);
    bool fin = isfinite(gdx) && isfinite(gdy);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        st_f64<NT>(th[i], col + (int64_t)(2 + 2 * i) * n_env);
        st_f64<NT>(thd[i], col + (int64_t)(3 + 2 * i) * n_env);
        fin = fin && isfinite(th[i]) && isfinite(thd[i]);
    }
    return fin ? 0 : SW_STATUS_NONFINITE;
}

// Workgroups of kStepBlock that cover n transitions (environments): the grid, and the length of a row of partials.
__host__ __device__ inline int64_t step_blocks(int64_t n) { return n <= 0 ? 0 : (n + kStepBlock - 1) / kStepBlock; }

// A stored transition: state, action and the stored next state (whose loads are in flight while the step is
// computed).  A lane that holds no transition (!live) gets zeros and reads nothing.
template <int N, bool NT>
__device__ __forceinline__ void load_transition(bool live, int64_t n_env, int64_t e, const double *__restrict__ sin_,
                                                const double *__restrict__ act, const double *__restrict__ next_ref,
                                                double &gdx, double &gdy, double (&th)[N], double (&thd)[N],
                                                double (&u)[N - 1], double &rx, double &ry, double (&rth)[N],
                                                double (&rthd)[N])
{
    gdx = gdy = rx = ry = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) th[i] = thd[i] = rth[i] = rthd[i] = 0.0;
#pragma unroll
    for (int i = 0; i < N - 1; ++i) u[i] = 0.0;
    if (live) {
        load_state<N, NT>(sin_, n_env, e, gdx, gdy, th, thd);
        load_action<N, NT>(act, n_env, e, u);
        load_state<N, NT>(next_ref, n_env, e, rx, ry, rth, rthd);
    }
}

// Inside sincos_fast's range?  Outside it every result is NaN (SW_STATUS_RANGE where there is a status).
template <int N> __device__ __forceinline__ bool angles_in_range(const double (&th)[N])
{
    return sw::track_angle_range<N>(0.0, th) < sw::kAngleLimit;
}

// One step in place with the range rule; returns the status word but for SW_STATUS_NONFINITE, which store_state adds.
template <int N, bool TWIN>
__device__ __forceinline__ int32_t step_checked(const sw::Consts &C, const sw::TwinConsts &T, double &gdx, double &gdy,
                                                double (&th)[N], double (&thd)[N], const double (&u)[N - 1], double &r)
{
    const bool in_range = angles_in_range<N>(th);
    const bool ok = TWIN ? sw::twin_step<N>(T, gdx, gdy, th, thd, u, r)
                         : sw::euler_step<N>(C, gdx, gdy, th, thd, u, r);
    if (!in_range) {   // outside sincos_fast's range: NaN out, SW_STATUS_RANGE
        gdx = gdy = r = __builtin_nan("");
#pragma unroll
        for (int i = 0; i < N; ++i) th[i] = thd[i] = __builtin_nan("");
    }
    return (ok ? 0 : SW_STATUS_SINGULAR) | (in_range ? 0 : SW_STATUS_RANGE);
}

// The accelerations with the range rule.
template <int N, bool TWIN>
__device__ __forceinline__ void accel_checked(const sw::Consts &C, const sw::TwinConsts &T, double gdx, double gdy,
                                              const double (&th)[N], const double (&thd)[N], const double (&u)[N - 1],
                                              double &ax, double &ay, double (&a)[N])
{
    const bool in_range = angles_in_range<N>(th);
    if (TWIN) sw::accelerations_twin<N>(T, gdx, gdy, th, thd, u, ax, ay, a);
    else sw::accelerations<N>(C, gdx, gdy, th, thd, u, ax, ay, a);
    if (!in_range) {
        ax = ay = __builtin_nan("");
#pragma unroll
        for (int i = 0; i < N; ++i) a[i] = __builtin_nan("");
    }
}

// || state - stored next state ||^2: one product, then an FMA chain over the components in the state's order.
template <int N>
__device__ __forceinline__ double residual_sq(double gdx, double gdy, const double (&th)[N], const double (&thd)[N],
                                              double rx, double ry, const double (&rth)[N], const double (&rthd)[N])
{
    double q = (gdx - rx) * (gdx - rx);
    q = __builtin_fma(gdy - ry, gdy - ry, q);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        q = __builtin_fma(th[i] - rth[i], th[i] - rth[i], q);
        q = __builtin_fma(thd[i] - rthd[i], thd[i] - rthd[i], q);
    }
    return q;
}

// The fixed-order sums.  wave_sum: the 64 lanes by shuffle tree (lane 0 has the sum).  post_wave_sum: a workgroup's
// value goes to w[wave]; behind a barrier waves_in_order adds those left to right.  row_sum: lane l adds
// row[l], row[l + 64], ... in turn (starting from 0.0), then the 64 lane sums go through the tree.
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

__device__ __forceinline__ void post_wave_sum(double v, double *w)
{
    v = wave_sum(v);
    if (threadIdx.x % kWave == 0) w[threadIdx.x / kWave] = v;
}

__device__ __forceinline__ double waves_in_order(const double *w)
{
    double t = w[0];
#pragma unroll
    for (int i = 1; i < kStepBlock / kWave; ++i) t += w[i];
    return t;
}

__device__ __forceinline__ double row_sum(const double *__restrict__ row, int64_t nb)
{
    double t = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += kWave) t += row[b];
    return wave_sum(t);
}

// A candidate x = [l_i, m_i, k] on top of the base parameters' h and direction: its consts, and whether it keeps
// validate_params' rule (a candidate that does not scores NaN, SW_STATUS_PARAM).
template <int N>
__device__ __forceinline__ bool candidate_setup(const sw::Consts &base, const double *__restrict__ x, sw::Consts &c)
{
    const double l = x[0], m = x[1], k = x[2];
    c = sw::consts_of(N, l, m, k, base.h, base.dirx, base.diry);
    return sim_params_ok(l, m, k);
}

// Candidates [c, c1) scored on the transition this lane holds: per candidate a copy of the state is stepped and
// its distance summed over the workgroup's waves into wsum[k] -- everything step_residual_kernel does for one.
template <int N>
__device__ __forceinline__ void score_candidates(int c, int c1, const sw::Consts *cc, const int *cok, bool live,
                                                 bool in_range, double gdx, double gdy, const double (&th)[N],
                                                 const double (&thd)[N], const double (&u)[N - 1], double rx,
                                                 double ry, const double (&rth)[N], const double (&rthd)[N],
                                                 double (*wsum)[kStepBlock / kWave])
{
#pragma unroll 1
    for (int k = c; k < c1; ++k) {
        double dist = 0.0;
        if (live) {
            double x = gdx, y = gdy, t[N], td[N], r;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                t[i] = th[i];
                td[i] = thd[i];
            }
            (void)sw::euler_step<N>(cc[k], x, y, t, td, u, r);
            const double q = residual_sq<N>(x, y, t, td, rx, ry, rth, rthd);
            dist = (in_range && cok[k]) ? sqrt(q) : __builtin_nan("");
        }
        post_wave_sum(dist, wsum[k]);
    }
}

template <int N, bool TWIN, bool NT>
__global__ void __launch_bounds__(kStepBlock)
step_kernel(sw::Consts C, sw::TwinConsts T, int64_t n_env, const double *__restrict__ sin_,
            const double *__restrict__ act, double *__restrict__ sout,
            double *__restrict__ reward, int32_t *__restrict__ status)
{
    const int64_t e = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    if (e >= n_env) return;
    double gdx, gdy, th[N], thd[N], u[N - 1], r;
    load_state<N, NT>(sin_, n_env, e, gdx, gdy, th, thd);
    load_action<N, NT>(act, n_env, e, u);
    int32_t word = step_checked<N, TWIN>(C, T, gdx, gdy, th, thd, u, r);
    word |= store_state<N, NT>(sout, n_env, e, gdx, gdy, th, thd);
    if (reward) st_f64<NT>(r, &reward[e]);
    if (status) status[e] = word;
}

// One physics step per stored transition, COMPARED with the stored next state instead of written out: the
// estimator's objective I(x) (ars/estimator.py:36-62) is the sum over every stored transition of
// || sim_step(s_t, a_t) - s_{t+1} ||_2.  Reads state + action + stored next state (16 d + 8 m bytes per transition),
// writes ONE double per workgroup: the fixed-order sum of its transitions' distances (lanes by shuffle tree, the four
// waves in order) -- deterministic, and the d doubles per transition the step kernel would store, the difference
// kernel would read back and the norm kernel would reduce never exist.  Out-of-range angles give NaN (as in step_kernel).
template <int N, bool NT>
__global__ void __launch_bounds__(kStepBlock)
step_residual_kernel(sw::Consts C, int64_t n_env, const double *__restrict__ sin_, const double *__restrict__ act,
                     const double *__restrict__ next_ref, double *__restrict__ partial)
{
    __shared__ double wsum[kStepBlock / kWave];
    const int64_t e = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    double dist = 0.0;
    if (e < n_env) {
        double gdx, gdy, th[N], thd[N], u[N - 1], rx, ry, rth[N], rthd[N], r;
        load_transition<N, NT>(true, n_env, e, sin_, act, next_ref, gdx, gdy, th, thd, u, rx, ry, rth, rthd);
        const bool in_range = angles_in_range<N>(th);
        (void)sw::euler_step<N>(C, gdx, gdy, th, thd, u, r);
        const double q = residual_sq<N>(gdx, gdy, th, thd, rx, ry, rth, rthd);
        dist = in_range ? sqrt(q) : __builtin_nan("");
    }
    post_wave_sum(dist, wsum);
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = waves_in_order(wsum);
}

// The same objective for a POPULATION of parameter sets (the CMA-ES generation of the estimator's search): each
// workgroup reads its 256 transitions ONCE into registers and steps a copy of every state for each candidate of its
// group (blockIdx.y: candidates [y * kPopGroup, ...)).  Per candidate everything is step_residual_kernel's: the same
// partition, the same consts (sw::consts_of, here from the candidate's l_i, m_i, k), euler_step, the same FMA chain, the
// same lane tree and wave order -- partial[j][b] has the bits step_residual_kernel gives for candidate j.  A candidate
// that breaks validate_params' rule gets NaN partials and SW_STATUS_PARAM; its neighbours do not notice.
template <int N, bool NT>
__global__ void __launch_bounds__(kStepBlock)
step_residual_pop_kernel(sw::Consts base, int64_t n_cand, const double *__restrict__ cand, int64_t n_env,
                         const double *__restrict__ sin_, const double *__restrict__ act,
                         const double *__restrict__ next_ref, double *__restrict__ partial,
                         int32_t *__restrict__ cand_status)
{
    __shared__ sw::Consts cc[kPopGroup];
    __shared__ int cok[kPopGroup];
    __shared__ double wsum[kPopGroup][kStepBlock / kWave];
    const int64_t j0 = (int64_t)blockIdx.y * kPopGroup;
    const int nc = (int)(n_cand - j0 < kPopGroup ? n_cand - j0 : kPopGroup);
    if ((int)threadIdx.x < nc) {
        const bool ok = candidate_setup<N>(base, cand + (j0 + threadIdx.x) * 3, cc[threadIdx.x]);
        cok[threadIdx.x] = ok;
        if (cand_status && blockIdx.x == 0) cand_status[j0 + threadIdx.x] = ok ? SW_STATUS_OK : SW_STATUS_PARAM;
    }
    const int64_t e = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    const bool live = e < n_env;
    double gdx, gdy, th[N], thd[N], u[N - 1], rx, ry, rth[N], rthd[N];
    load_transition<N, NT>(live, n_env, e, sin_, act, next_ref, gdx, gdy, th, thd, u, rx, ry, rth, rthd);
    const bool in_range = angles_in_range<N>(th);
    __syncthreads();
    score_candidates<N>(0, nc, cc, cok, live, in_range, gdx, gdy, th, thd, u, rx, ry, rth, rthd, wsum);
    __syncthreads();
    if ((int)threadIdx.x < nc)
        partial[(j0 + threadIdx.x) * (int64_t)gridDim.x + blockIdx.x] = waves_in_order(wsum[threadIdx.x]);
}

// value[j] = the sum of row j of partial [n_cand][nb] in row_sum's order.  One wave per candidate.
__global__ void __launch_bounds__(kWave)
residual_rows_sum_kernel(int64_t nb, const double *__restrict__ partial, double *__restrict__ value)
{
    const double t = row_sum(partial + (int64_t)blockIdx.x * nb, nb);
    if (threadIdx.x == 0) value[blockIdx.x] = t;
}

// Columns [b0, b0 + len) of set s of the concatenated transitions (set_begin [n_set + 1], ascending).  False for a set
// index or bounds that do not fit the arrays the host sized (n_set, n_env, the row stride from max_set_len): such a
// set is never read and nothing is written for it.
__device__ __forceinline__ bool set_span(const int64_t *__restrict__ set_begin, int64_t s, int64_t n_set, int64_t n_env,
                                         int64_t max_set_len, int64_t &b0, int64_t &len)
{
    b0 = len = 0;
    if (s < 0 || s >= n_set) return false;
    const int64_t a = set_begin[s], b = set_begin[s + 1];
    if (a < 0 || b > n_env || b <= a || b - a > max_set_len) return false;
    b0 = a;
    len = b - a;
    return true;
}

// step_residual_pop_kernel for candidates that do not all score on the same transitions (a batch of estimators in
// lock-step): candidate j scores on set cand_set[j] of the concatenated transitions.  blockIdx.x counts 256-transition
// blocks FROM THE SET'S FIRST COLUMN, so per candidate everything is step_residual_kernel's on the set alone: partition,
// consts, euler_step, FMA chain, lane tree, wave order.  A workgroup reads its transitions once for each run of
// same-set candidates of its group (cand_set ascending: one run per set); a run whose set ends before this block is
// skipped, and a workgroup beyond the longest set of its group returns before the first barrier (both tests are
// workgroup-uniform).  partial is [n_cand][gridDim.x]; row j's entries beyond its set's last block are not written.
template <int N>
__global__ void __launch_bounds__(kStepBlock)
step_residual_sets_kernel(sw::Consts base, int64_t n_set, const int64_t *__restrict__ set_begin, int64_t max_set_len,
                          int64_t n_cand, const double *__restrict__ cand, const int32_t *__restrict__ cand_set,
                          int64_t n_env, const double *__restrict__ sin_, const double *__restrict__ act,
                          const double *__restrict__ next_ref, double *__restrict__ partial,
                          int32_t *__restrict__ cand_status)
{
    __shared__ sw::Consts cc[kPopGroup];
    __shared__ int cok[kPopGroup];
    __shared__ int64_t cbeg[kPopGroup], clen[kPopGroup];
    __shared__ int32_t cset[kPopGroup];
    __shared__ double wsum[kPopGroup][kStepBlock / kWave];
    const int64_t j0 = (int64_t)blockIdx.y * kPopGroup;
    const int nc = (int)(n_cand - j0 < kPopGroup ? n_cand - j0 : kPopGroup);
    const int64_t t0 = (int64_t)blockIdx.x * kStepBlock;   // this block's first transition, counted inside a set
    int64_t longest = 0;
    for (int c = 0; c < nc; ++c) {   // uniform
        int64_t b0, len;
        (void)set_span(set_begin, cand_set[j0 + c], n_set, n_env, max_set_len, b0, len);
        longest = len > longest ? len : longest;
    }
    if ((int)threadIdx.x < nc) {
        const bool ok = candidate_setup<N>(base, cand + (j0 + threadIdx.x) * 3, cc[threadIdx.x]);
        cok[threadIdx.x] = ok;
        if (cand_status && blockIdx.x == 0) cand_status[j0 + threadIdx.x] = ok ? SW_STATUS_OK : SW_STATUS_PARAM;
        if (t0 < longest) {
            const int32_t s = cand_set[j0 + threadIdx.x];
            cset[threadIdx.x] = s;
            (void)set_span(set_begin, s, n_set, n_env, max_set_len, cbeg[threadIdx.x], clen[threadIdx.x]);
        }
    }
    if (t0 >= longest) return;   // beyond every set of this group (uniform, in front of the barriers)
    __syncthreads();
    int c = 0;
    while (c < nc) {             // one trip per run of same-set candidates (uniform)
        int c1 = c + 1;
        while (c1 < nc && cset[c1] == cset[c]) ++c1;
        const int64_t len = clen[c];
        if (t0 < len) {
            const bool live = t0 + threadIdx.x < len;
            double gdx, gdy, th[N], thd[N], u[N - 1], rx, ry, rth[N], rthd[N];
            load_transition<N, false>(live, n_env, cbeg[c] + t0 + threadIdx.x, sin_, act, next_ref, gdx, gdy, th, thd,
                                      u, rx, ry, rth, rthd);
            score_candidates<N>(c, c1, cc, cok, live, angles_in_range<N>(th), gdx, gdy, th, thd, u, rx, ry, rth, rthd,
                                wsum);
        }
        c = c1;
    }
    __syncthreads();
    if ((int)threadIdx.x < nc && t0 < clen[threadIdx.x])
        partial[(j0 + threadIdx.x) * (int64_t)gridDim.x + blockIdx.x] = waves_in_order(wsum[threadIdx.x]);
}

// residual_rows_sum_kernel for rows of different lengths: row r of partial [gridDim.x][stride] belongs to set
// row_set[r] (nullptr: to set r / rows_per_set) and holds one entry per 256-transition block of that set; value[r] =
// their sum in row_sum's order.  A set with active[s] == 0, or with bounds that do not fit, is skipped.
__global__ void __launch_bounds__(kWave)
residual_set_rows_sum_kernel(int64_t n_set, const int64_t *__restrict__ set_begin, int64_t max_set_len, int64_t n_env,
                             const int32_t *__restrict__ row_set, int rows_per_set, const int32_t *__restrict__ active,
                             int64_t stride, const double *__restrict__ partial, double *__restrict__ value)
{
    const int64_t s = row_set ? (int64_t)row_set[blockIdx.x] : (int64_t)(blockIdx.x / rows_per_set);
    int64_t b0, len;
    if (!set_span(set_begin, s, n_set, n_env, max_set_len, b0, len)) return;
    if (active && !active[s]) return;
    const double t = row_sum(partial + (int64_t)blockIdx.x * stride, step_blocks(len));
    if (threadIdx.x == 0) value[blockIdx.x] = t;
}

// The least-squares refinement's normal equations for many transition sets at once (Estimator._residual_normal /
// _residual_cost for a batch of estimators): workgroup (b, s) steps block b of set s at NP parameter points
// (points [n_set][NP][3] = l_i, m_i, k; NP = 7: centre, +e0, -e0, +e1, -e1, +e2, -e2), forms the residual vectors r =
// step - next_ref in registers and, with 7 points, the central-difference columns J_i = (r_+i - r_-i) inv_2e[s][i],
// and sums K = 1 (r.r) or 13 (r.r | J^T J row-major | J^T r) values over its transitions in a fixed order: FMA chain
// over the d components, lanes by shuffle tree, the four waves in order.  partial [n_set][K][gridDim.x]; the simulated
// states never reach memory.  Out-of-range angles, or a point that breaks the parameter rule, make the sums NaN.
template <int N, int NP>
__global__ void __launch_bounds__(kStepBlock)
step_residual_normal_sets_kernel(sw::Consts base, int64_t n_set, const int64_t *__restrict__ set_begin,
                                 int64_t max_set_len, const double *__restrict__ points,
                                 const double *__restrict__ inv_2e, const int32_t *__restrict__ active, int64_t n_env,
                                 const double *__restrict__ sin_, const double *__restrict__ act,
                                 const double *__restrict__ next_ref, double *__restrict__ partial,
                                 int32_t *__restrict__ set_status)
{
    constexpr int D = 2 * N + 2, K = NP == 7 ? 13 : 1;
    static_assert(NP == 1 || NP == 7, "one point (cost) or seven (normal equations)");
    __shared__ sw::Consts cc[NP];
    __shared__ int cok[NP];
    __shared__ double wsum[K][kStepBlock / kWave];
    const int64_t s = blockIdx.y, t0 = (int64_t)blockIdx.x * kStepBlock;
    int64_t b0, len;
    if (!set_span(set_begin, s, n_set, n_env, max_set_len, b0, len)) return;   // uniform, in front of the barriers
    if (active && !active[s]) return;
    if (t0 >= len) return;
    if ((int)threadIdx.x < NP)
        cok[threadIdx.x] = candidate_setup<N>(base, points + (s * NP + threadIdx.x) * 3, cc[threadIdx.x]);
    const bool live = t0 + threadIdx.x < len;
    double gdx, gdy, th[N], thd[N], u[N - 1], rx, ry, rth[N], rthd[N];
    load_transition<N, false>(live, n_env, b0 + t0 + threadIdx.x, sin_, act, next_ref, gdx, gdy, th, thd, u, rx, ry,
                              rth, rthd);
    const bool in_range = angles_in_range<N>(th);
    double ie[3] = {0.0, 0.0, 0.0};
    if (NP == 7) {
#pragma unroll
        for (int i = 0; i < 3; ++i) ie[i] = inv_2e[s * 3 + i];
    }
    __syncthreads();
    bool ok = in_range;
    double r0[D], rp[D], J0[D], J1[D], J2[D];
#pragma unroll
    for (int i = 0; i < D; ++i) r0[i] = rp[i] = J0[i] = J1[i] = J2[i] = 0.0;
#pragma unroll 1
    for (int p = 0; p < NP; ++p) {   // one copy of the step's code; the point's role is a uniform choice
        double x = gdx, y = gdy, t[N], td[N], rew, rt[D];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            t[i] = th[i];
            td[i] = thd[i];
        }
        (void)sw::euler_step<N>(cc[p], x, y, t, td, u, rew);
        ok = ok && cok[p];
        rt[0] = x - rx;
        rt[1] = y - ry;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            rt[2 + 2 * i] = t[i] - rth[i];
            rt[3 + 2 * i] = td[i] - rthd[i];
        }
        if (p == 0) {
#pragma unroll
            for (int i = 0; i < D; ++i) r0[i] = rt[i];
        } else if (p & 1) {
#pragma unroll
            for (int i = 0; i < D; ++i) rp[i] = rt[i];
        } else {
            const double inv = p == 2 ? ie[0] : p == 4 ? ie[1] : ie[2];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const double j = (rp[i] - rt[i]) * inv;
                J0[i] = p == 2 ? j : J0[i];
                J1[i] = p == 4 ? j : J1[i];
                J2[i] = p == 6 ? j : J2[i];
            }
        }
    }
    double acc[K];
#pragma unroll
    for (int v = 0; v < K; ++v) acc[v] = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        acc[0] = __builtin_fma(r0[i], r0[i], acc[0]);
        if (NP == 7) {
            acc[1] = __builtin_fma(J0[i], J0[i], acc[1]);
            acc[2] = __builtin_fma(J0[i], J1[i], acc[2]);
            acc[3] = __builtin_fma(J0[i], J2[i], acc[3]);
            acc[5] = __builtin_fma(J1[i], J1[i], acc[5]);
            acc[6] = __builtin_fma(J1[i], J2[i], acc[6]);
            acc[9] = __builtin_fma(J2[i], J2[i], acc[9]);
            acc[10] = __builtin_fma(J0[i], r0[i], acc[10]);
            acc[11] = __builtin_fma(J1[i], r0[i], acc[11]);
            acc[12] = __builtin_fma(J2[i], r0[i], acc[12]);
        }
    }
    if (NP == 7) {   // J^T J is symmetric: the lower triangle is the upper one's bits
        acc[4] = acc[2];
        acc[7] = acc[3];
        acc[8] = acc[6];
    }
#pragma unroll
    for (int v = 0; v < K; ++v) post_wave_sum(live ? (ok ? acc[v] : __builtin_nan("")) : 0.0, wsum[v]);
    __syncthreads();
    if ((int)threadIdx.x < K)
        partial[(s * K + threadIdx.x) * (int64_t)gridDim.x + blockIdx.x] = waves_in_order(wsum[threadIdx.x]);
    if (set_status && blockIdx.x == 0 && threadIdx.x == 0) {
        bool all = true;
        for (int p = 0; p < NP; ++p) all = all && cok[p];
        set_status[s] = all ? SW_STATUS_OK : SW_STATUS_PARAM;
    }
}

template <int N, bool TWIN>
__global__ void __launch_bounds__(kStepBlock)
accel_kernel(sw::Consts C, sw::TwinConsts T, int64_t n_env, const double *__restrict__ sin_,
             const double *__restrict__ act, double *__restrict__ gdd, double *__restrict__ tdd)
{
    const int64_t e = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    if (e >= n_env) return;
    double gdx, gdy, th[N], thd[N], u[N - 1], a[N], ax, ay;
    load_state<N, false>(sin_, n_env, e, gdx, gdy, th, thd);
    load_action<N, false>(act, n_env, e, u);
    accel_checked<N, TWIN>(C, T, gdx, gdy, th, thd, u, ax, ay, a);
    gdd[e] = ax;
    gdd[n_env + e] = ay;
#pragma unroll
    for (int i = 0; i < N; ++i) tdd[(int64_t)i * n_env + e] = a[i];
}

// Gym reset: Gdot = 0, theta = pi/2, thetadot = 0 (remy_swimmer_env.py:64-66); the native
// twin's env_start sets every observation entry to 0.001 (SwimmerEnvironment.cpp:39-42).
__global__ void reset_kernel(int n, int twin, int64_t n_env, double *__restrict__ state)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    state[e] = twin ? kTwinStart : 0.0;
    state[n_env + e] = twin ? kTwinStart : 0.0;
    for (int i = 0; i < n; ++i) {
        state[(int64_t)(2 + 2 * i) * n_env + e] = twin ? kTwinStart : kHalfPi;
        state[(int64_t)(3 + 2 * i) * n_env + e] = twin ? kTwinStart : 0.0;
    }
}

// One swimmer handed over in HOST memory (sw_env1, the batch-1 drop-in surfaces).  io = the
// handle's pinned, device-mapped block (SW_ENV1_* offsets).  One wave: lane l pulls double l of
// [state | action] -- ONE read burst over the bus instead of 25 round trips -- every lane then
// runs the same step on broadcast copies (step_checked / accel_checked: the batched kernels' bits), lane 0 posts
// the results and, behind a system-scope fence, the sequence number the host spins on.
template <int N, bool TWIN, bool ACCEL>
__global__ void __launch_bounds__(kWave)
env1_kernel(sw::Consts C, sw::TwinConsts T, double *__restrict__ io, int32_t *__restrict__ status,
            uint32_t *__restrict__ seq_flag, uint32_t seq)
{
    constexpr int D = 2 * N + 2, M = N - 1;
    const int lane = threadIdx.x;
    const double mine = (lane < SW_ENV1_ACTION + M) ? io[lane] : 0.0;   // state 0..17, action 18..24
    double gdx = __shfl(mine, 0, kWave), gdy = __shfl(mine, 1, kWave);
    double th[N], thd[N], u[M];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        th[i] = __shfl(mine, 2 + 2 * i, kWave);
        thd[i] = __shfl(mine, 3 + 2 * i, kWave);
    }
#pragma unroll
    for (int i = 0; i < M; ++i) u[i] = __shfl(mine, SW_ENV1_ACTION + i, kWave);
    if (ACCEL) {
        double ax, ay, a[N];
        accel_checked<N, TWIN>(C, T, gdx, gdy, th, thd, u, ax, ay, a);
        if (lane == 0) {
            io[SW_ENV1_GDD] = ax;
            io[SW_ENV1_GDD + 1] = ay;
#pragma unroll
            for (int i = 0; i < N; ++i) io[SW_ENV1_TDD + i] = a[i];
        }
    } else {
        double r;
        const int32_t word = step_checked<N, TWIN>(C, T, gdx, gdy, th, thd, u, r);
        if (lane == 0) {   // the next state is a batch of one: rows at stride 1
            *status = word | store_state<N, false>(io + SW_ENV1_NEXT, 1, 0, gdx, gdy, th, thd);
            io[SW_ENV1_REWARD] = r;
        }
    }
    static_assert(D <= SW_ENV1_ACTION && SW_ENV1_ACTION + M <= SW_ENV1_NEXT && SW_ENV1_NEXT + D <= SW_ENV1_REWARD,
                  "I/O block layout");
    if (lane == 0) {
        __threadfence_system();   // the results are visible to the host before the sequence number is
        __hip_atomic_store(seq_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Batches beyond the Infinity Cache stream through HBM: the step kernels' NT (nontemporal) forms.
bool streams_through_hbm(const sw_params *p, int64_t n_env)
{
    const int d = 2 * p->n + 2;
    return n_env * (int64_t)(8 * (2 * d + p->n)) > kStepStreamBytes;
}

bool any_null(std::initializer_list<const void *> pointers)
{
    for (const void *p : pointers)
        if (!p) return true;
    return false;
}

// The argument check of the population, sets and normal-equations entries, which all decide in this order: the base
// parameters (check_params, which also clears stale launch errors), a missing array, a size out of range, then a
// model or a point count that has no kernel.
int check_residual_batch(const sw_params *base, bool null_array, bool bad_size, bool bad_choice = false)
{
    const int rc = check_params(base);
    if (rc) return rc;
    if (null_array) return SW_ERR_NULL;
    if (bad_size) return SW_ERR_SIZE;
    return is_twin(base) || bad_choice ? SW_ERR_PARAM : SW_OK;   // the objective is defined on the Gym model
}

// The end of those entries, behind the launch of the kernel that writes the partials (known_n: with_n found one):
// its status and, where the caller wants the sums, the launch of the row sums behind it.
template <class Launch> int then_row_sums(bool known_n, bool wanted, Launch &&launch_row_sums)
{
    if (!known_n) return SW_ERR_SEGMENTS;
    if (wanted) {
        const int rc = launch_status();
        if (rc) return rc;
        launch_row_sums();
    }
    return launch_status();
}

}  // namespace

extern "C" {

int sw_reset_f64(const sw_params *p, int64_t n_env, double *state, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (!state) return SW_ERR_NULL;
    if (n_env < 0) return SW_ERR_SIZE;
    if (n_env == 0) return SW_OK;
    const unsigned grid = (unsigned)((n_env + 255) / 256);
    hipLaunchKernelGGL(reset_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p->n,
                       is_twin(p) ? 1 : 0, n_env, state);
    return launch_status();
}

int sw_step_f64(const sw_params *p, int64_t n_env, const double *state_in, const double *action,
                double *state_out, double *reward, int32_t *status, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (n_env < 0) return SW_ERR_SIZE;
    if (n_env == 0) return SW_OK;
    if (!state_in || !action || !state_out) return SW_ERR_NULL;
    const sw::Consts C = make_consts(p);
    const sw::TwinConsts T = make_twin_consts(p);
    bool nt = streams_through_hbm(p, n_env);
    static const char *nt_env = getenv("SWIMMER_STEP_NT");   // measurement knob: "0" / "1" force it
    if (nt_env && (nt_env[0] == '0' || nt_env[0] == '1')) nt = nt_env[0] == '1';
    auto launch = [&](auto *kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)step_blocks(n_env)), dim3(kStepBlock), 0, (hipStream_t)stream, C, T,
                           n_env, state_in, action, state_out, reward, status);
    };
    // (the twin model has no nontemporal form)
    const bool known_n =
        is_twin(p) ? with_n<2, 8>(p->n, [&](auto N) { launch(step_kernel<N.value, true, false>); })
                   : with_n<2, 8>(p->n, [&](auto N, auto NT) { launch(step_kernel<N.value, false, NT.value>); }, nt);
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

int sw_step_residual_f64(const sw_params *p, int64_t n_env, const double *state, const double *action,
                         const double *next_ref, double *partial, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (is_twin(p)) return SW_ERR_PARAM;          // the estimator's objective is defined on the Gym model
    if (n_env < 0) return SW_ERR_SIZE;
    if (n_env == 0) return SW_OK;
    if (!state || !action || !next_ref || !partial) return SW_ERR_NULL;
    const sw::Consts C = make_consts(p);
    const bool known_n = with_n<2, 8>(p->n, [&](auto N, auto NT) {
        hipLaunchKernelGGL((step_residual_kernel<N.value, NT.value>), dim3((unsigned)step_blocks(n_env)),
                           dim3(kStepBlock), 0, (hipStream_t)stream, C, n_env, state, action, next_ref, partial);
    }, streams_through_hbm(p, n_env));
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

int sw_step_residual_pop_f64(const sw_params *base, int64_t n_cand, const double *cand, int64_t n_env,
                             const double *state, const double *action, const double *next_ref, double *partial,
                             double *value, int32_t *cand_status, void *stream)
{
    const int rc = check_residual_batch(base, any_null({cand, state, action, next_ref, partial}),
                                        n_cand < 1 || n_cand > kPopMaxCandidates || n_env < 0);
    if (rc) return rc;
    if (n_env == 0) return SW_OK;
    const sw::Consts C = make_consts(base);    // h and the direction; l_i, m_i, k come from each candidate
    const int64_t nb = step_blocks(n_env);
    const dim3 grid((unsigned)nb, (unsigned)((n_cand + kPopGroup - 1) / kPopGroup));
    const bool known_n = with_n<2, 8>(base->n, [&](auto N, auto NT) {
        hipLaunchKernelGGL((step_residual_pop_kernel<N.value, NT.value>), grid, dim3(kStepBlock), 0,
                           (hipStream_t)stream, C, n_cand, cand, n_env, state, action, next_ref, partial,
                           cand_status);
    }, streams_through_hbm(base, n_env));
    return then_row_sums(known_n, value != nullptr, [&] {
        hipLaunchKernelGGL(residual_rows_sum_kernel, dim3((unsigned)n_cand), dim3(kWave), 0, (hipStream_t)stream, nb,
                           partial, value);
    });
}

int sw_step_residual_sets_f64(const sw_params *base, int64_t n_set, const int64_t *set_begin, int64_t max_set_len,
                              int64_t n_cand, const double *cand, const int32_t *cand_set, int64_t n_env,
                              const double *state, const double *action, const double *next_ref, double *partial,
                              double *value, int32_t *cand_status, void *stream)
{
    const int rc = check_residual_batch(base, any_null({set_begin, cand, cand_set, state, action, next_ref, partial}),
                                        n_set < 1 || n_cand < 1 || n_cand > kPopMaxCandidates || max_set_len < 1 ||
                                            n_env < 1 || max_set_len > n_env);
    if (rc) return rc;
    const sw::Consts C = make_consts(base);    // h and the direction; l_i, m_i, k come from each candidate
    const int64_t nb = step_blocks(max_set_len);
    const dim3 grid((unsigned)nb, (unsigned)((n_cand + kPopGroup - 1) / kPopGroup));
    const bool known_n = with_n<2, 8>(base->n, [&](auto N) {
        hipLaunchKernelGGL((step_residual_sets_kernel<N.value>), grid, dim3(kStepBlock), 0, (hipStream_t)stream, C,
                           n_set, set_begin, max_set_len, n_cand, cand, cand_set, n_env, state, action, next_ref,
                           partial, cand_status);
    });
    return then_row_sums(known_n, value != nullptr, [&] {
        hipLaunchKernelGGL(residual_set_rows_sum_kernel, dim3((unsigned)n_cand), dim3(kWave), 0, (hipStream_t)stream,
                           n_set, set_begin, max_set_len, n_env, cand_set, 1, (const int32_t *)nullptr, nb, partial,
                           value);
    });
}

int sw_step_residual_normal_sets_f64(const sw_params *base, int64_t n_set, const int64_t *set_begin,
                                     int64_t max_set_len, int32_t n_point, const double *points, const double *inv_2e,
                                     const int32_t *active, int64_t n_env, const double *state, const double *action,
                                     const double *next_ref, double *partial, double *out, int32_t *set_status,
                                     void *stream)
{
    const int rc = check_residual_batch(
        base, any_null({set_begin, points, state, action, next_ref, partial, out}) || (n_point == 7 && !inv_2e),
        n_set < 1 || n_set > kSetsMax || max_set_len < 1 || n_env < 1 || max_set_len > n_env,
        n_point != 1 && n_point != 7);
    if (rc) return rc;
    const sw::Consts C = make_consts(base);
    const int64_t nb = step_blocks(max_set_len);
    const dim3 grid((unsigned)nb, (unsigned)n_set);
    const bool known_n = with_n<2, 8>(base->n, [&](auto N, auto NORMAL) {
        hipLaunchKernelGGL((step_residual_normal_sets_kernel<N.value, NORMAL.value ? 7 : 1>), grid, dim3(kStepBlock),
                           0, (hipStream_t)stream, C, n_set, set_begin, max_set_len, points, inv_2e, active, n_env,
                           state, action, next_ref, partial, set_status);
    }, n_point == 7);
    const int K = n_point == 7 ? 13 : 1;
    return then_row_sums(known_n, true, [&] {
        hipLaunchKernelGGL(residual_set_rows_sum_kernel, dim3((unsigned)(n_set * K)), dim3(kWave), 0,
                           (hipStream_t)stream, n_set, set_begin, max_set_len, n_env, (const int32_t *)nullptr, K,
                           active, nb, partial, out);
    });
}

int64_t sw_step_residual_blocks(int64_t n_env) { return step_blocks(n_env); }

int sw_accel_f64(const sw_params *p, int64_t n_env, const double *state, const double *action,
                 double *gdd, double *tdd, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (n_env < 0) return SW_ERR_SIZE;
    if (n_env == 0) return SW_OK;
    if (!state || !action || !gdd || !tdd) return SW_ERR_NULL;
    const sw::Consts C = make_consts(p);
    const sw::TwinConsts T = make_twin_consts(p);
    const bool known_n = with_n<2, 8>(p->n, [&](auto N, auto TWIN) {
        hipLaunchKernelGGL((accel_kernel<N.value, TWIN.value>), dim3((unsigned)step_blocks(n_env)), dim3(kStepBlock),
                           0, (hipStream_t)stream, C, T, n_env, state, action, gdd, tdd);
    }, is_twin(p));
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

// ---- one swimmer per call (include/swimmer_hip.h, sw_env1) -----------------------------
struct sw_env1 {
    double *io_host = nullptr, *io_dev = nullptr;   // SW_ENV1_DOUBLES doubles + {status, seq}
    hipStream_t stream = nullptr;
    uint32_t seq = 0;
    int device = 0;   // the device that was current at sw_env1_create: every launch goes there
};

int sw_env1_create(sw_env1 **out)
{
    if (!out) return SW_ERR_NULL;
    sw_env1 *e = new (std::nothrow) sw_env1();
    if (!e) return SW_ERR_LAUNCH;
    const size_t bytes = sizeof(double) * SW_ENV1_DOUBLES + 64;
    bool ok = hipGetDevice(&e->device) == hipSuccess;
    ok = ok && hipHostMalloc((void **)&e->io_host, bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
    if (ok) {
        memset(e->io_host, 0, bytes);
        ok = hipHostGetDevicePointer((void **)&e->io_dev, e->io_host, 0) == hipSuccess &&
             hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) == hipSuccess;
        // (normal priority: a batch-1 step has nothing to overtake)
    }
    if (!ok) {
        sw_env1_destroy(e);
        return SW_ERR_LAUNCH;
    }
    *out = e;
    return SW_OK;
}

void sw_env1_destroy(sw_env1 *e)
{
    if (!e) return;
    if (e->stream) {
        (void)hipStreamSynchronize(e->stream);
        (void)hipStreamDestroy(e->stream);
    }
    if (e->io_host) (void)hipHostFree(e->io_host);
    delete e;
}

double *sw_env1_io(sw_env1 *e) { return e ? e->io_host : nullptr; }

static int env1_run(sw_env1 *e, const sw_params *p, bool accel, int32_t *status)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (!e) return SW_ERR_NULL;
    const sw::Consts C = make_consts(p);
    const sw::TwinConsts T = make_twin_consts(p);
    int32_t *st_host = reinterpret_cast<int32_t *>(e->io_host + SW_ENV1_DOUBLES);
    int32_t *st_dev = reinterpret_cast<int32_t *>(e->io_dev + SW_ENV1_DOUBLES);
    const volatile uint32_t *flag_host = reinterpret_cast<const volatile uint32_t *>(st_host + 1);
    uint32_t *flag_dev = reinterpret_cast<uint32_t *>(st_dev + 1);
    const uint32_t seq = ++e->seq;
    // the handle's stream and mapped block belong to e->device: launch there whatever the caller's current
    // device is, and leave the caller's current device as it was
    int caller_device = e->device;
    if (hipGetDevice(&caller_device) != hipSuccess) return SW_ERR_LAUNCH;
    if (caller_device != e->device && hipSetDevice(e->device) != hipSuccess) return SW_ERR_LAUNCH;
    const bool known_n = with_n<2, 8>(p->n, [&](auto N, auto TWIN, auto ACCEL) {
        hipLaunchKernelGGL((env1_kernel<N.value, TWIN.value, ACCEL.value>), dim3(1), dim3(kWave), 0, e->stream, C, T,
                           e->io_dev, st_dev, flag_dev, seq);
    }, is_twin(p), accel);
    rc = known_n ? launch_status() : SW_ERR_SEGMENTS;
    if (caller_device != e->device) (void)hipSetDevice(caller_device);
    if (rc) return rc;
    for (int64_t spins = 0; *flag_host != seq; ++spins) {
        if ((spins & 0xffff) == 0xffff) {
            // not hot any more: a stream that has drained without the flag moving has failed
            const hipError_t q = hipStreamQuery(e->stream);
            if (q == hipSuccess) {
                if (*flag_host == seq) break;
                return SW_ERR_LAUNCH;
            }
            if (q != hipErrorNotReady) return SW_ERR_LAUNCH;
        }
        __builtin_ia32_pause();
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (status) *status = accel ? 0 : *st_host;
    return SW_OK;
}

int sw_env1_step(sw_env1 *e, const sw_params *p, int32_t *status) { return env1_run(e, p, false, status); }
int sw_env1_accel(sw_env1 *e, const sw_params *p) { return env1_run(e, p, true, nullptr); }

}  // extern "C"
