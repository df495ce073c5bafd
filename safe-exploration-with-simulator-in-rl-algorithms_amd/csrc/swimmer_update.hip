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
#include "swimmer_update.inc"
}

// sw_ars_update_multi_f64: ars_update_kernel for n_agent agents in one launch, grid (m*d + 1, n_agent).  Workgroup
// (e, a) does for agent a what workgroup e of the single kernel does: the same body on the agent's slices (world = 1
// view of its returns and moment rows), so each agent's result has the bits a single sw_ars_update_f64 call gives.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
ars_update_multi_kernel(int d, int md, int32_t n_dir, int32_t n_rows, const double *__restrict__ returns_all,
                        const double *__restrict__ moments_all, const double *__restrict__ deltas_all,
                        double *__restrict__ policy_all, double alpha, double b, int64_t top_b,
                        double *__restrict__ running_all, double n_new, double *__restrict__ mean_all,
                        double *__restrict__ inv_std_all, double *__restrict__ sigma_all)
{
    const int64_t agent = blockIdx.y;
    const GatherView gv{returns_all + agent * 2 * n_dir,
                        moments_all ? moments_all + agent * n_rows * (2 * d) : nullptr, 0, n_dir, n_rows, 1};
    const double *__restrict__ const deltas = deltas_all + agent * n_dir * md;
    double *__restrict__ const policy = policy_all + agent * md;
    double *__restrict__ const running = running_all ? running_all + agent * (1 + 2 * d) : nullptr;
    double *__restrict__ const mean = mean_all ? mean_all + agent * d : nullptr;
    double *__restrict__ const inv_std = inv_std_all ? inv_std_all + agent * d : nullptr;
    double *__restrict__ const sigma_out = sigma_all ? sigma_all + agent : nullptr;
#include "swimmer_update.inc"
}

// sw_ars_update_multi_counted_f64: ars_update_multi_kernel with every agent's direction count read on the device.
// n_dir_max and n_rows_max set the strides; agent a runs the body with n_dir = count[a], top_b clamped to it, its
// ceil(2 count[a] / 16) written moment rows and n_new = 2 count[a] H -- the arguments of the single-agent call with
// n_dir = count[a], whose order of summation depends on n_dir only.  An agent with count 0 is left untouched.  The
// body's order also depends on the workgroup size, which the single-agent call picks from n_dir: a launch serves the
// agents whose count picks ITS size and returns for the others (the entry point launches both sizes when n_dir_max
// reaches the wide one).  Both tests are workgroup-uniform and sit in front of every barrier.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
ars_update_counted_kernel(int d, int md, int32_t n_dir_max, int32_t n_rows_max, const int32_t *__restrict__ count,
                          const double *__restrict__ returns_all, const double *__restrict__ moments_all,
                          const double *__restrict__ deltas_all, double *__restrict__ policy_all, double alpha,
                          double b, int64_t top_b_max, double *__restrict__ running_all, int32_t H,
                          double *__restrict__ mean_all, double *__restrict__ inv_std_all,
                          double *__restrict__ sigma_all)
{
    const int64_t agent = blockIdx.y;
    const int32_t counted = __builtin_amdgcn_readfirstlane(count[agent]);
    const int32_t n_dir = counted < 0 ? 0 : (counted > n_dir_max ? n_dir_max : counted);
    if (n_dir == 0 || (n_dir >= kUpdWideFrom) != (BLOCK == kUpdBlockWide)) return;
    const int32_t n_rows = (2 * n_dir + kMomGroup - 1) / kMomGroup;
    const int64_t top_b = top_b_max < n_dir ? top_b_max : n_dir;
    const double n_new = (double)(2 * (int64_t)n_dir * H);
    const GatherView gv{returns_all + agent * 2 * n_dir_max,
                        moments_all ? moments_all + agent * n_rows_max * (2 * d) : nullptr, 0, n_dir, n_rows, 1};
    const double *__restrict__ const deltas = deltas_all + agent * n_dir_max * md;
    double *__restrict__ const policy = policy_all + agent * md;
    double *__restrict__ const running = running_all ? running_all + agent * (1 + 2 * d) : nullptr;
    double *__restrict__ const mean = mean_all ? mean_all + agent * d : nullptr;
    double *__restrict__ const inv_std = inv_std_all ? inv_std_all + agent * d : nullptr;
    double *__restrict__ const sigma_out = sigma_all ? sigma_all + agent : nullptr;
#include "swimmer_update.inc"
}

// sw_ars_pack_admitted_f64: one workgroup per agent turns the gate's admit flags [n_dir] (and, where given, its status
// [2 n_dir]: a direction with a failed simulator rollout counts as refused) into the agent's count, the admitted
// indices in ascending order (entries count.. are -1) and the admitted deltas packed in that order.  The position of
// an admitted direction is a prefix sum over the flags: ballot + popcount inside a wave, the waves' totals through
// LDS, 256 directions per round -- no atomics, the same output whatever the waves' timing.
constexpr int kPackBlock = 256;

__global__ void __launch_bounds__(kPackBlock)
ars_pack_admitted_kernel(int32_t n_dir, int md, const int32_t *__restrict__ admit_all,
                         const int32_t *__restrict__ status_all, const double *__restrict__ deltas_all,
                         int32_t *__restrict__ count, int32_t *__restrict__ order_all,
                         double *__restrict__ packed_all)
{
    constexpr int NW = kPackBlock / kWave;
    __shared__ int32_t wave_total[NW];
    const int64_t agent = blockIdx.x;
    const int32_t *admit = admit_all + agent * n_dir;
    const int32_t *status = status_all ? status_all + agent * 2 * n_dir : nullptr;
    int32_t *order = order_all + agent * n_dir;
    const int w = threadIdx.x / kWave, l = threadIdx.x % kWave;
    int32_t done = 0;   // admitted directions in front of this round (uniform)
    for (int32_t i0 = 0; i0 < n_dir; i0 += kPackBlock) {
        const int32_t i = i0 + (int32_t)threadIdx.x;
        bool in = false;
        if (i < n_dir) {
            in = admit[i] != 0;
            if (status) in = in && status[2 * i] == 0 && status[2 * i + 1] == 0;
        }
        const unsigned long long votes = __ballot(in);
        const int32_t before = __popcll(votes & ((1ull << l) - 1ull));
        if (l == 0) wave_total[w] = __popcll(votes);
        __syncthreads();
        int32_t base = done, round = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            base += (k < w) ? wave_total[k] : 0;
            round += wave_total[k];
        }
        if (in) order[base + before] = i;
        done += round;
        __syncthreads();   // wave_total is rewritten in the next round
    }
    for (int32_t j = done + (int32_t)threadIdx.x; j < n_dir; j += kPackBlock) order[j] = -1;
    if (threadIdx.x == 0) count[agent] = done;
    __threadfence_block();
    __syncthreads();   // the workgroup's own stores to `order` are read below
    const double *deltas = deltas_all + agent * n_dir * md;
    double *packed = packed_all + agent * n_dir * md;
    const int64_t total = (int64_t)done * md;
    for (int64_t x = threadIdx.x; x < total; x += kPackBlock) {
        const int64_t j = x / md, e = x - j * md;
        packed[x] = deltas[(int64_t)order[j] * md + e];
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

int sw_ars_update_multi_f64(const sw_params *p, int64_t n_agent, int64_t n_dir, const double *returns,
                            const double *deltas, double *policy, double alpha, double b, int64_t top_b,
                            const double *moments, int64_t n_moment_rows, double *running,
                            int64_t n_new_states, double *mean, double *inv_std, double *sigma_out,
                            void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (n_agent < 1 || n_agent > 65535 || n_dir <= 0 || n_dir > INT32_MAX / 4 || n_moment_rows < 0 ||
        n_moment_rows > INT32_MAX || n_new_states < 0)
        return SW_ERR_SIZE;
    if (!returns || !deltas || !policy) return SW_ERR_NULL;
    if (running && (!moments || !mean || !inv_std)) return SW_ERR_NULL;
    const int d = 2 * p->n + 2, md = (p->n - 1) * d;
    // block size by n_dir, as launch_update: the order of summation is the single-agent call's
    with_bools([&](auto WIDE) {
        constexpr int kBlock = WIDE.value ? kUpdBlockWide : kUpdBlock;
        hipLaunchKernelGGL(ars_update_multi_kernel<kBlock>, dim3(md + 1, (unsigned)n_agent), dim3(kBlock), 0,
                           (hipStream_t)stream, d, md, (int32_t)n_dir, (int32_t)n_moment_rows, returns, moments,
                           deltas, policy, alpha, b, top_b, running, (double)n_new_states, mean, inv_std, sigma_out);
    }, n_dir >= kUpdWideFrom);
    return launch_status();
}

int sw_ars_update_multi_counted_f64(const sw_params *p, int64_t n_agent, int64_t n_dir, const int32_t *count,
                                    int32_t H, const double *returns, const double *deltas, double *policy,
                                    double alpha, double b, int64_t top_b, const double *moments,
                                    int64_t n_moment_rows, double *running, double *mean, double *inv_std,
                                    double *sigma_out, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (n_agent < 1 || n_agent > 65535 || n_dir < 1 || n_dir > INT32_MAX / 4 || H < 0 || n_moment_rows < 0 ||
        n_moment_rows > INT32_MAX || top_b < 0 || (int64_t)2 * n_dir * H > ((int64_t)1 << 52))
        return SW_ERR_SIZE;
    if (!count || !returns || !deltas || !policy) return SW_ERR_NULL;
    if (running && (!moments || !mean || !inv_std)) return SW_ERR_NULL;
    if (running && n_moment_rows < (2 * n_dir + kMomGroup - 1) / kMomGroup) return SW_ERR_SIZE;
    const int d = 2 * p->n + 2, md = (p->n - 1) * d;
    // one launch per workgroup size the counts can pick (ars_update_counted_kernel): the wide one only from
    // kUpdWideFrom directions
    const dim3 grid(md + 1, (unsigned)n_agent);
    hipLaunchKernelGGL(ars_update_counted_kernel<kUpdBlock>, grid, dim3(kUpdBlock), 0, (hipStream_t)stream, d, md,
                       (int32_t)n_dir, (int32_t)n_moment_rows, count, returns, moments, deltas, policy, alpha, b, top_b,
                       running, H, mean, inv_std, sigma_out);
    if (n_dir >= kUpdWideFrom)
        hipLaunchKernelGGL(ars_update_counted_kernel<kUpdBlockWide>, grid, dim3(kUpdBlockWide), 0, (hipStream_t)stream,
                           d, md, (int32_t)n_dir, (int32_t)n_moment_rows, count, returns, moments, deltas, policy, alpha,
                           b, top_b, running, H, mean, inv_std, sigma_out);
    return launch_status();
}

int sw_ars_pack_admitted_f64(const sw_params *p, int64_t n_agent, int64_t n_dir, const int32_t *admit,
                             const int32_t *status, const double *deltas, int32_t *count, int32_t *order,
                             double *packed, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (n_agent < 1 || n_agent > 65535 || n_dir < 1 || n_dir > INT32_MAX / 4) return SW_ERR_SIZE;
    if (!admit || !deltas || !count || !order || !packed) return SW_ERR_NULL;
    const int d = 2 * p->n + 2, md = (p->n - 1) * d;
    hipLaunchKernelGGL(ars_pack_admitted_kernel, dim3((unsigned)n_agent), dim3(kPackBlock), 0, (hipStream_t)stream,
                       (int32_t)n_dir, md, admit, status, deltas, count, order, packed);
    return launch_status();
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
