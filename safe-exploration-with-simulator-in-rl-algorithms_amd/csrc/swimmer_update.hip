// swimmer_update.hip -- the ARS update between two rollout launches: sigma_R, the policy step and the merge of the
// V2 statistics in one kernel, reading the iteration's results where the all-gather left them.
#include "swimmer_launch.h"

namespace {

// ------------------------------------------------------------------------------------
// two sums with one pair of barriers (the update kernel is pure latency: every barrier counts)
template <int BLOCK>
__device__ __forceinline__ void block_sum2(double &a, double &b, double (*sh2)[2])
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        a += __shfl_down(a, off, kWave);
        b += __shfl_down(b, off, kWave);
    }
    const int w = threadIdx.x / kWave, l = threadIdx.x % kWave;
    __syncthreads();
    if (l == 0) {
        sh2[w][0] = a;
        sh2[w][1] = b;
    }
    __syncthreads();
    double ta = 0.0, tb = 0.0;
    for (int i = 0; i < BLOCK / kWave; ++i) {
        ta += sh2[i][0];
        tb += sh2[i][1];
    }
    a = ta;
    b = tb;
}

// Where the update finds an iteration's results.  After the all-gather every rank's segment
// [2*chunk returns | rows_chunk moment rows] sits at rank*seg_len in one buffer; the kernel
// indexes that layout directly so no repacking kernels run between the collective and the
// update.  Separate returns / moments arrays are the world = 1 special case.
struct GatherView {
    const double *ret_base;
    const double *mom_base;
    int64_t seg_len;      // doubles between consecutive ranks' segments
    int32_t chunk;        // direction slots per rank
    int32_t rows_chunk;   // moment rows per rank
    int32_t world;
};

__device__ __forceinline__ double ret_at(const GatherView &g, int32_t dir, int sign_idx)
{
    const int32_t rank = dir / g.chunk, local = dir - rank * g.chunk;
    return g.ret_base[rank * g.seg_len + 2 * local + sign_idx];
}

// used(i): all directions (top_b == 0) or the top_b by max(r+, r-), ties to the higher index
// (argsort ascending, reversed: ars_agent.py:105-108).  With top_b active every workgroup first
// stages the N keys in LDS and ranks them there (N^2 / 256 comparisons per thread), leaving a
// byte mask; directions beyond the LDS capacity fall back to ranking from global memory.
constexpr int kTopBMaxDirs = 6144;   // 48 KB of keys + 6 KB of flags

__device__ __forceinline__ bool rank_used_global(const GatherView &g, int32_t n_dir, int64_t top_b, int32_t i)
{
    const double ki = fmax(ret_at(g, i, 0), ret_at(g, i, 1));
    int64_t rank = 0;
    for (int32_t j = 0; j < n_dir; ++j) {
        const double kj = fmax(ret_at(g, j, 0), ret_at(g, j, 1));
        rank += (kj > ki) || (kj == ki && j > i);
    }
    return rank < top_b;
}

// grid = m*d + 1 workgroups.  Workgroup e < m*d updates policy entry e; the last one merges
// the V2 statistics.  The kernel sits on the critical path between two rollout launches and
// is pure latency, so every workgroup first pulls what it needs with ONE round of loads (the
// 2 n_dir returns and its delta column into LDS / registers; all moment rows in parallel) and
// then only touches LDS: ~5 us instead of ~17 us for the load-then-use-per-pass version.
constexpr int kUpdMaxDirs = kTopBMaxDirs;
constexpr int kTopBSortDirs = 2048;   // top-b by a bitonic sort in LDS up to here, by ranking beyond

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
ars_update_kernel(int d, int md, int32_t n_dir, GatherView gv,
                  const double *__restrict__ deltas, double *__restrict__ policy, double alpha,
                  double b, int64_t top_b, double *__restrict__ running, double n_new,
                  double *__restrict__ mean, double *__restrict__ inv_std,
                  double *__restrict__ sigma_out)
{
    __shared__ double sh2[BLOCK / kWave][2];
    __shared__ double rp_s[kUpdMaxDirs], rm_s[kUpdMaxDirs];   // r+ and r- of every direction
    __shared__ unsigned char flag[kUpdMaxDirs];
    const int e = blockIdx.x;
    if (e < md) {
        const bool select = top_b > 0 && top_b < n_dir;
        const bool in_lds = n_dir <= kUpdMaxDirs;
        // one round of global loads: returns -> LDS, this workgroup's delta column -> registers
        constexpr int kMaxPer = (kUpdMaxDirs + BLOCK - 1) / BLOCK;
        double dcol[kMaxPer];
        if (in_lds) {
#pragma unroll
            for (int q = 0; q < kMaxPer; ++q) {
                const int32_t i = threadIdx.x + q * BLOCK;
                dcol[q] = (i < n_dir) ? deltas[(int64_t)i * md + e] : 0.0;
            }
            for (int32_t i = threadIdx.x; i < n_dir; i += BLOCK) {
                rp_s[i] = ret_at(gv, i, 0);
                rm_s[i] = ret_at(gv, i, 1);
            }
            __syncthreads();
            if (select && n_dir <= kTopBSortDirs) {
                // Up to 2048 directions: a bitonic sort of (key, index) in LDS, best first -- key = max(r+, r-)
                // descending, ties to the higher index, NaN keys first (np.argsort puts NaN last and the reference
                // reverses it, ars_agent.py:105-108).  log2(P) (log2(P) + 1) / 2 compare-exchange stages of P / 2
                // pairs each (45 stages at 512 directions: ~4 us) instead of N^2 / BLOCK comparisons per thread with
                // the key list re-read for every direction (~25 us on the critical path between two rollout launches).
                __shared__ double skey[kTopBSortDirs];
                __shared__ uint16_t sidx[kTopBSortDirs];
                uint32_t P2 = 2;
                while (P2 < (uint32_t)n_dir) P2 <<= 1;
                for (uint32_t i = threadIdx.x; i < P2; i += BLOCK) {
                    double k = -HUGE_VAL;
                    if (i < (uint32_t)n_dir) {
                        // NOT fmax: Python's max(a, b) = (b > a) ? b : a (safe_ars / ars_agent sort_directions)
                        const double a = rp_s[i], b = rm_s[i];
                        k = (b > a) ? b : a;
                        k = (k != k) ? HUGE_VAL : k;
                    }
                    skey[i] = k;
                    sidx[i] = (uint16_t)i;
                }
                __syncthreads();
                for (uint32_t k = 2; k <= P2; k <<= 1) {
                    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                        for (uint32_t t = threadIdx.x; t < P2 / 2; t += BLOCK) {
                            const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
                            const double ka = skey[lo], kb = skey[hi];
                            const uint32_t ia = sidx[lo], ib = sidx[hi];
                            // a goes before b?  padding (index >= n_dir) always goes last
                            const bool a_first = (ia < (uint32_t)n_dir) &&
                                                 ((ib >= (uint32_t)n_dir) || ka > kb || (ka == kb && ia > ib));
                            const bool best_first = (lo & k) == 0;     // direction of this bitonic block
                            if (a_first != best_first) {
                                skey[lo] = kb;
                                skey[hi] = ka;
                                sidx[lo] = (uint16_t)ib;
                                sidx[hi] = (uint16_t)ia;
                            }
                        }
                        __syncthreads();
                    }
                }
                for (uint32_t pos = threadIdx.x; pos < P2; pos += BLOCK) {
                    const uint32_t i = sidx[pos];
                    if (i < (uint32_t)n_dir) flag[i] = (int64_t)pos < top_b;
                }
                __syncthreads();
            } else if (select) {
                for (int32_t i = threadIdx.x; i < n_dir; i += BLOCK) {
                    const double ki = fmax(rp_s[i], rm_s[i]);
                    int32_t rank = 0;
                    for (int32_t j = 0; j < n_dir; ++j) {
                        const double kj = fmax(rp_s[j], rm_s[j]);
                        rank += (kj > ki) || (kj == ki && j > i);
                    }
                    flag[i] = rank < top_b;
                }
                __syncthreads();
            }
        }
        auto rplus = [&](int32_t i) { return in_lds ? rp_s[i] : ret_at(gv, i, 0); };
        auto rminus = [&](int32_t i) { return in_lds ? rm_s[i] : ret_at(gv, i, 1); };
        auto dir_used = [&](int32_t i) -> bool {
            if (!select) return true;
            return in_lds ? (flag[i] != 0) : rank_used_global(gv, n_dir, top_b, i);
        };
        // np.std(used_rewards): two-pass, ddof = 0 (ars_agent.py:123)
        double s = 0.0, cnt = 0.0;
        for (int32_t i = threadIdx.x; i < n_dir; i += BLOCK)
            if (dir_used(i)) {
                s += rplus(i) + rminus(i);
                cnt += 2.0;
            }
        block_sum2<BLOCK>(s, cnt, sh2);
        const double mu = s / cnt;
        double v = 0.0, g = 0.0;
        if (in_lds) {
#pragma unroll   // static index into dcol[] (a runtime index would send it to scratch)
            for (int q = 0; q < kMaxPer; ++q) {
                const int32_t i = threadIdx.x + q * BLOCK;
                if (i < n_dir && dir_used(i)) {
                    const double rp = rp_s[i], rm = rm_s[i];
                    const double a = rp - mu, c = rm - mu;
                    v += a * a + c * c;
                    g = __builtin_fma(rp - rm, dcol[q], g);
                }
            }
        } else {
            for (int32_t i = threadIdx.x; i < n_dir; i += BLOCK)
                if (dir_used(i)) {
                    const double rp = rplus(i), rm = rminus(i);
                    const double a = rp - mu, c = rm - mu;
                    v += a * a + c * c;
                    g = __builtin_fma(rp - rm, deltas[(int64_t)i * md + e], g);
                }
        }
        block_sum2<BLOCK>(v, g, sh2);
        if (threadIdx.x == 0) {
            const double sigma = sqrt(v / cnt);
            // divisor: b as given (ars_agent.py:128: all directions used, b only divides), or with
            // a true top-b truncation the number of directions used, len(order) (safe_ars/ars.py:64)
            const double div = (top_b > 0) ? 0.5 * cnt : b;
            const double grad = g / (div * sigma);
            policy[e] = policy[e] + alpha * grad;           // ars_agent.py:130
            if (e == 0 && sigma_out) *sigma_out = sigma;
        }
    } else if (running != nullptr) {
        // V2 statistics over every state seen since training began (np.mean / np.cov with
        // ddof = 1, ars_agent.py:179-182).  The reference recomputes them two-pass over the
        // whole (ever-growing) list; here `running` = {n, mean - c, M2 = sum (x - mean)^2} and
        // each iteration's batch is MERGED into it (Chan et al.): the batch's own mean and M2
        // come from its sums about the pivot c (reset state; every rollout starts there, so
        // |mean_b - c| is never large against the batch's spread), and the merge itself adds
        // non-negative terms only -- no cancellation that grows with the length of training.
        // The workgroup's 256 threads form G = 256 / 2d row groups x 2d columns: thread (rg, j) sums
        // column j over the rows whose GLOBAL index (rank-major) is congruent to rg mod G, in
        // ascending order, eight loads in flight per round (one round up to 8 G rows: 128 rows for
        // n = 3) -- the loop used to run over 4 row groups only and paid one memory latency per 16
        // rows, 4 rounds at 512 directions.  The G partial sums are added in ascending group
        // order.  Global row indices make the grouping -- and every bit of the result --
        // independent of the world size for row-aligned shards, and identical on every rank.
        constexpr int kMaxCols = 2 * (2 * SW_MAX_SEGMENTS + 2);     // 2d <= 36
        constexpr int kMaxGroups = BLOCK / 12;                  // 2d >= 12 (n = 2): G <= 21 (16 for n = 3)
        __shared__ double part[kMaxGroups][kMaxCols];
        __shared__ double bsum[kMaxCols];
        const int cols = 2 * d, G = BLOCK / cols;
        const int rg = threadIdx.x / cols, j = threadIdx.x - rg * cols;
        const int32_t total = gv.world * gv.rows_chunk;
        if (rg < G) {
            double acc = 0.0;
            for (int32_t g0 = rg; g0 < total; g0 += 8 * G) {
                double v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int32_t g = g0 + q * G;
                    v[q] = 0.0;
                    if (g < total) {
                        const int32_t r = g / gv.rows_chunk, row = g - r * gv.rows_chunk;
                        v[q] = gv.mom_base[r * gv.seg_len + (int64_t)row * cols + j];
                    }
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) acc += v[q];
            }
            part[rg][j] = acc;
        }
        __syncthreads();
        if (threadIdx.x < cols) {
            double t = part[0][threadIdx.x];
            for (int g = 1; g < G; ++g) t += part[g][threadIdx.x];
            bsum[threadIdx.x] = t;
        }
        __syncthreads();
        const double n0 = running[0], n1 = n0 + n_new;
        if (threadIdx.x < d && n_new > 0.0) {
            const int c_ = threadIdx.x;
            const double s1 = bsum[c_], s2 = bsum[d + c_];
            const double mb = s1 / n_new;                       // batch mean - c
            const double m2b = __builtin_fma(-s1, mb, s2);      // batch sum (x - mean_b)^2
            const double mr = running[1 + c_], m2 = running[1 + d + c_];
            const double delta = mb - mr;
            const double mr1 = __builtin_fma(delta, n_new / n1, mr);
            const double m21 = (m2 + m2b) + delta * delta * (n0 * (n_new / n1));
            running[1 + c_] = mr1;
            running[1 + d + c_] = m21;
            const double c = (c_ >= 2 && (c_ & 1) == 0) ? kHalfPi : 0.0;
            mean[c_] = c + mr1;
            inv_std[c_] = 1.0 / sqrt(m21 / (n1 - 1.0));          // diag(cov) ** -0.5
        }
        __syncthreads();
        if (threadIdx.x == 0) running[0] = n1;
    }
}

}  // namespace

extern "C" {

static int launch_update(const sw_params *p, int64_t n_dir, const GatherView &gv,
                         const double *deltas, double *policy, double alpha, double b,
                         int64_t top_b, double *running, int64_t n_new_states, double *mean,
                         double *inv_std, double *sigma_out, void *stream)
{
    const int d = 2 * p->n + 2, md = (p->n - 1) * d;
    // The kernel is pure latency between two rollout launches; a thread's share of the directions (and of
    // the moment rows) sets it.  256 threads per workgroup up to 1024 directions, 1024 beyond: 2048
    // directions 11.6 -> ~6 us (rocprofv3).  The summation order is a function of n_dir only, so every
    // rank of a sharded run and the single-process run of the same problem still get the same bits.
    with_bools([&](auto WIDE) {
        constexpr int kBlock = WIDE.value ? kUpdBlockWide : kUpdBlock;
        hipLaunchKernelGGL(ars_update_kernel<kBlock>, dim3(md + 1), dim3(kBlock), 0, (hipStream_t)stream, d, md,
                           (int32_t)n_dir, gv, deltas, policy, alpha, b, top_b, running, (double)n_new_states,
                           mean, inv_std, sigma_out);
    }, n_dir >= kUpdWideFrom);
    return launch_status();
}

int sw_ars_update_f64(const sw_params *p, int64_t n_dir, const double *returns,
                      const double *deltas, double *policy, double alpha, double b, int64_t top_b,
                      const double *moments, int64_t n_moment_rows, double *running,
                      int64_t n_new_states, double *mean, double *inv_std, double *sigma_out,
                      void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (n_dir <= 0 || n_dir > INT32_MAX / 4 || n_moment_rows < 0 || n_moment_rows > INT32_MAX ||
        n_new_states < 0)
        return SW_ERR_SIZE;
    if (!returns || !deltas || !policy) return SW_ERR_NULL;
    if (running && (!moments || !mean || !inv_std)) return SW_ERR_NULL;
    const GatherView gv{returns, moments, 0, (int32_t)n_dir, (int32_t)n_moment_rows, 1};
    return launch_update(p, n_dir, gv, deltas, policy, alpha, b, top_b, running, n_new_states,
                         mean, inv_std, sigma_out, stream);
}

int sw_ars_update_gathered_f64(const sw_params *p, int64_t n_dir, const double *gathered,
                               int32_t world, int64_t chunk, int64_t rows_chunk,
                               const double *deltas, double *policy, double alpha, double b,
                               int64_t top_b, double *running, int64_t n_new_states, double *mean,
                               double *inv_std, double *sigma_out, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (n_dir <= 0 || n_dir > INT32_MAX / 4 || world < 1 || chunk < 1 || rows_chunk < 0 ||
        chunk > INT32_MAX / 4 || rows_chunk > INT32_MAX || (int64_t)world * chunk < n_dir ||
        n_new_states < 0)
        return SW_ERR_SIZE;
    if (!gathered || !deltas || !policy) return SW_ERR_NULL;
    if (running && (!mean || !inv_std)) return SW_ERR_NULL;
    const int d = 2 * p->n + 2;
    const int64_t seg_len = 2 * chunk + rows_chunk * 2 * d;
    const GatherView gv{gathered, gathered + 2 * chunk, seg_len, (int32_t)chunk,
                        (int32_t)rows_chunk, world};
    return launch_update(p, n_dir, gv, deltas, policy, alpha, b, top_b, running, n_new_states,
                         mean, inv_std, sigma_out, stream);
}

}  // extern "C"
