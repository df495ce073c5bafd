// swimmer_cov.h -- the covariance pass over a trajectory buffer as device code: one tile of it (moments_tile), run
// by the standalone traj_moments_kernel (swimmer_cov.hip) and by the extra workgroups that ride along in a launch of
// the segment-per-lane rollout kernels (SideJob; swimmer_rollout_n3.hip, swimmer_rollout_row.hip), and the launch of
// such a kernel with its side job.
#pragma once
#include "swimmer_launch.h"

namespace {

// Long chains (D >= 12, n >= 5) in 256-thread workgroups: the D (D + 1) / 2 + D sums do not fit one
// lane's registers, so the four waves of the workgroup work on the SAME 64 rollouts and split the
// sums between them (moments_split): a tile is 64 rollouts wide and four times as long.
__host__ __device__ constexpr bool cov_split(int D, int block) { return D >= 12 && block >= 256; }

// acc buffer of a covariance pass: [count | sum x (D) | sum x x^T (D x D)] followed by the
// pass's scratch: one ticket counter (a double slot whose first 4 bytes are the counter; all-zero
// bits = 0) and one row of D + D*D partial sums per tile.
__host__ __device__ constexpr int cov_sums(int D) { return 1 + D + D * D; }

// One tile of the full first / second moment sums of a trajectory buffer [H][D][n_roll]:
// BLOCK rollouts x the steps [t0, t1) (x = state - reset pivot), written to the tile's scratch
// row.  NO atomics on the sums: the tile that finishes last (ticket counter) adds all rows to acc
// in tile order, so the result does not depend on the order the tiles ran in.  Workgroups of any
// size that is a multiple of 64 can run it: the standalone traj_moments_kernel and the covariance
// workgroups that ride along in a rollout launch (SideJob).  For long chains the upper triangle is
// accumulated JB rows at a time (re-reading the tile from cache) so that the accumulators stay in
// registers.
// A tile's row of partial sums inside the pass's scratch.  The scratch is stored TRANSPOSED -- entry j of
// tile i at [j * n_tiles + i] -- so that the merge reads one entry of consecutive tiles with consecutive
// lanes (moments_tile); a tile's own stores are strided (fire and forget).
struct TileRow {
    double *p;
    int64_t stride;
    // agent-scope store (written through the XCD's L2): visible to the merging workgroup on another XCD once
    // the store has completed, without a write-back of everything else that is dirty in this L2
    __device__ __forceinline__ void put(int j, double v) const
    {
        __hip_atomic_store(p + (int64_t)j * stride, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

template <int D, int BLOCK, int J0, int JB>
__device__ __forceinline__ void moments_pass(int64_t n_roll, const double *__restrict__ traj,
                                             const TileRow tile_row, int64_t bx, int32_t t0, int32_t t1,
                                             double *sh /* [BLOCK / 64][D + JB * D] */)
{
    constexpr int NW = BLOCK / kWave, W = D + JB * D;
    constexpr int J1 = (J0 + JB < D) ? J0 + JB : D;   // rows [J0, J1) of the upper triangle
    const int64_t r = bx * BLOCK + threadIdx.x;
    const int w = threadIdx.x / kWave, l = threadIdx.x % kWave;
    double s1[D], s2[JB][D];
#pragma unroll
    for (int j = 0; j < D; ++j) s1[j] = 0.0;
#pragma unroll
    for (int a = 0; a < JB; ++a)
#pragma unroll
        for (int g = 0; g < D; ++g) s2[a][g] = 0.0;
    if (r < n_roll) {
        for (int32_t t = t0; t < t1; ++t) {
            const double *tp = traj + (int64_t)t * D * n_roll + r;
            double x[D];
#pragma unroll
            for (int j = J0; j < D; ++j) {   // later passes need columns >= J0 only
                const double c = (j >= 2 && (j & 1) == 0) ? kHalfPi : 0.0;
                x[j] = tp[(int64_t)j * n_roll] - c;
            }
            if (J0 == 0) {
#pragma unroll
                for (int j = 0; j < D; ++j) s1[j] += x[j];
            }
#pragma unroll
            for (int f = J0; f < J1; ++f)
#pragma unroll
                for (int g = f; g < D; ++g) s2[f - J0][g] = __builtin_fma(x[f], x[g], s2[f - J0][g]);
        }
    }
    __syncthreads();   // the previous pass has drained sh
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const bool live = (j < D) ? (J0 == 0) : (J0 + (j - D) / D < J1 && (j - D) % D >= J0 + (j - D) / D);
        if (!live) continue;   // compile-time after unrolling
        double v = (j < D) ? s1[j < D ? j : 0] : s2[(j >= D ? j - D : 0) / D][(j >= D ? j - D : 0) % D];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
        if (l == 0) sh[w * W + j] = v;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < W; j += BLOCK) {
        const int f = J0 + (j - D) / D, g = (j - D) % D;
        const bool live = (j < D) ? (J0 == 0) : (f < J1 && g >= f);
        if (!live) continue;
        double v = 0.0;
        for (int i = 0; i < NW; ++i) v += sh[i * W + j];   // fixed order over the waves
        if (j < D) tile_row.put(j, v);
        else tile_row.put(D + f * D + g, v);                // upper triangle only
    }
}

template <int D, int BLOCK, int JB, int J0 = 0>
struct MomentsPasses {
    static __device__ __forceinline__ void run(int64_t n_roll, const double *__restrict__ traj,
                                               const TileRow tile_row, int64_t bx, int32_t t0,
                                               int32_t t1, double *sh)
    {
        if constexpr (J0 < D) {
            moments_pass<D, BLOCK, J0, JB>(n_roll, traj, tile_row, bx, t0, t1, sh);
            MomentsPasses<D, BLOCK, JB, J0 + JB>::run(n_roll, traj, tile_row, bx, t0, t1, sh);
        }
    }
};

// ---- long chains: the sums of a tile split over the four waves of the workgroup -----------------
// items 0 .. D-1 are the first moments, item D + p is pair p = (f, g), f <= g, of the upper triangle
// in row-major order.  Wave w owns items [w * PER, (w + 1) * PER): ~30 accumulators for D = 14
// instead of 119, so ONE pass over the tile suffices (the multi-pass form re-reads it 2-4 times),
// two steps' loads are in flight at a time, and the waves' loads of the same 64 rollouts hit in the
// vector L1 / L2 after the first one.  Each wave reduces its own sums over the lanes and writes them
// to the tile's row: no LDS, no barrier.
__host__ __device__ constexpr int pair_row(int D, int p)
{
    int f = 0;
    while (p >= D - f) {
        p -= D - f;
        ++f;
    }
    return f;
}
__host__ __device__ constexpr int pair_col(int D, int p)
{
    int f = 0;
    while (p >= D - f) {
        p -= D - f;
        ++f;
    }
    return f + p;
}

// item Q of the tile's sums, with every index a compile-time constant (a loop variable, even
// fully unrolled, left the pair lookup to the optimiser, which put x[] and acc[] in scratch)
template <int D, int Q>
__device__ __forceinline__ void moments_item_add(double &a, const double (&x)[D])
{
    if constexpr (Q < D) {
        a += x[Q];
    } else {
        constexpr int f = pair_row(D, Q - D), g = pair_col(D, Q - D);
        a = __builtin_fma(x[f], x[g], a);
    }
}

template <int D, int Q>
__device__ __forceinline__ void moments_item_store(double v, const TileRow tile_row)
{
    if constexpr (Q < D) {
        tile_row.put(Q, v);
    } else {
        constexpr int f = pair_row(D, Q - D), g = pair_col(D, Q - D);
        tile_row.put(D + f * D + g, v);   // upper triangle only
    }
}

template <int D, int WV, int... I>
__device__ __forceinline__ void moments_split_wave(int64_t n_roll, const double *__restrict__ traj,
                                                   const TileRow tile_row, int64_t r0, int32_t t0,
                                                   int32_t t1, int32_t nap, std::integer_sequence<int, I...>)
{
    constexpr int ITEMS = D + D * (D + 1) / 2, PER = (ITEMS + 3) / 4, Q0 = WV * PER;
    constexpr int CNT = (int)sizeof...(I);   // = min(PER, ITEMS - Q0)
    // the lowest state column this wave multiplies: columns below it are never loaded
    constexpr int JMIN = (Q0 < D) ? 0 : pair_row(D, Q0 - D);
    const int l = threadIdx.x % kWave;
    double acc[CNT];
#pragma unroll
    for (int q = 0; q < CNT; ++q) acc[q] = 0.0;
    // buffer loads: the step's slab base (wave-uniform, scalar arithmetic) is the resource's base, the
    // column is the scalar offset, the lane the 32-bit vector offset -- no per-lane 64-bit address
    // arithmetic in the loop.  One slab (D n_roll doubles) is < 4 GiB for every supported n_roll.
    const uint32_t lane_bytes = (uint32_t)l * 8u;
    const uint32_t col_bytes = (uint32_t)(n_roll * 8);
    auto load = [&](double (&x)[D], int32_t t) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<double *>(traj + ((int64_t)t * D * n_roll + r0)), 0, (int)0xffffffffu, 0x00020000);
#pragma unroll
        for (int j = JMIN; j < D; ++j) {
            const double c = (j >= 2 && (j & 1) == 0) ? kHalfPi : 0.0;
            typedef unsigned int v2u __attribute__((ext_vector_type(2)));
            union { v2u i; double d; } u;
            u.i = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)lane_bytes, (int)((uint32_t)j * col_bytes), 0);
            x[j] = u.d - c;
        }
    };
    if (r0 + l < n_roll && t0 < t1) {
        // THREE steps' loads in flight (a riding wave is alone with its memory latency: the tile's time is
        // steps x latency / depth), no conditionals in the steady state (they cost register copies).  Every
        // accumulator still adds its steps in order: the sums do not depend on the depth.
        double xa[D], xb[D], xc[D];
        auto add = [&](const double (&x)[D]) { (moments_item_add<D, Q0 + I>(acc[I], x), ...); };
        int32_t t = t0;
        load(xa, t);
        if (t + 1 < t1) load(xb, t + 1);
        for (; t + 4 < t1; t += 3) {     // xa, xb hold steps t, t + 1
            load(xc, t + 2);
            add(xa);
            load(xa, t + 3);
            add(xb);
            load(xb, t + 4);
            add(xc);
            for (int32_t z = 0; z < nap; ++z) __builtin_amdgcn_s_sleep(16);   // measurement knob (SWIMMER_COV_NAP)
        }
        const int32_t left = t1 - t;     // 1..4 steps, xa (and xb if left >= 2) loaded
        if (left >= 3) load(xc, t + 2);
        add(xa);
        if (left >= 4) load(xa, t + 3);
        if (left >= 2) add(xb);
        if (left >= 3) add(xc);
        if (left >= 4) add(xa);
    }
#pragma unroll
    for (int q = 0; q < CNT; ++q) {
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) acc[q] += __shfl_down(acc[q], off, kWave);
    }
    if (l == 0) (moments_item_store<D, Q0 + I>(acc[I], tile_row), ...);
}

template <int D, int WV>
__device__ __forceinline__ void moments_split_part(int64_t n_roll, const double *__restrict__ traj,
                                                   const TileRow tile_row, int64_t r0, int32_t t0, int32_t t1,
                                                   int32_t nap)
{
    constexpr int ITEMS = D + D * (D + 1) / 2, PER = (ITEMS + 3) / 4, Q0 = WV * PER;
    constexpr int CNT = (Q0 + PER <= ITEMS) ? PER : ITEMS - Q0;
    moments_split_wave<D, WV>(n_roll, traj, tile_row, r0, t0, t1, nap, std::make_integer_sequence<int, CNT>{});
}

template <int D>
__device__ __forceinline__ void moments_split(int64_t n_roll, const double *__restrict__ traj, const TileRow tile_row,
                                              int64_t bx, int32_t t0, int32_t t1, int32_t nap)
{
    const int64_t r0 = bx * kWave;
    switch (__builtin_amdgcn_readfirstlane(threadIdx.x / kWave)) {   // scalar: the waves' addresses stay uniform
    case 0: moments_split_part<D, 0>(n_roll, traj, tile_row, r0, t0, t1, nap); break;
    case 1: moments_split_part<D, 1>(n_roll, traj, tile_row, r0, t0, t1, nap); break;
    case 2: moments_split_part<D, 2>(n_roll, traj, tile_row, r0, t0, t1, nap); break;
    default: moments_split_part<D, 3>(n_roll, traj, tile_row, r0, t0, t1, nap); break;
    }
}

// Tile `tile` of `n_tiles` (tile = by * nbx + bx).  acc = [sums | counter | n_tiles rows].
template <int D, int BLOCK>
__device__ __forceinline__ void moments_tile(int64_t n_roll, int32_t H, const double *__restrict__ traj,
                                             double *__restrict__ acc, int64_t bx, int32_t t0, int32_t t1,
                                             uint32_t tile, uint32_t n_tiles, int32_t nap = 0)
{
    // rows of the upper triangle per pass: as many as keep the accumulators (D + the rows' entries)
    // plus one state inside 256 VGPRs -- one pass up to D = 12, 2 / 3 / 4 passes for D = 14 / 16 / 18
    constexpr int JB = (D <= 12) ? D : (D == 14 ? 7 : (D == 16 ? 6 : 5));
    constexpr int W = D + D * D;
    __shared__ uint32_t ticket;
    double *rows = acc + cov_sums(D) + 1;              // [W][n_tiles]
    const TileRow row{rows + tile, (int64_t)n_tiles};
    if constexpr (cov_split(D, BLOCK)) {
        static_assert(BLOCK == 4 * kWave, "moments_split: four waves per workgroup");
        moments_split<D>(n_roll, traj, row, bx, t0, t1, nap);
    } else {
        __shared__ double sh[(BLOCK / kWave) * (D + JB * D)];
        MomentsPasses<D, BLOCK, JB>::run(n_roll, traj, row, bx, t0, t1, sh);
    }
    // The row's stores are agent-scope write-through stores (TileRow::put): once they have COMPLETED the row is
    // visible device-wide.  Every wave therefore waits for its own stores (s_waitcnt vmcnt(0): a workgroup-scope
    // release fence does NOT emit that wait on gfx950) before the barrier behind which thread 0 takes the ticket,
    // so the ticket can never become visible before the row has reached memory.  No device-scope release
    // here: it would write back the whole L2 -- in a rollout launch that is the trajectories -- per tile.
    // (tests/test_isa_contracts.py checks the wait in the built code.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0)
        ticket = atomicAdd(reinterpret_cast<uint32_t *>(acc + cov_sums(D)), 1u);
    __syncthreads();
    if (ticket != n_tiles - 1u) return;
    // Last tile to finish: add every tile's row to acc.  The merge is a chain of memory latencies (the
    // rows were written by other XCDs: every load misses), so it is laid out for loads in flight, not
    // for arithmetic: a wave takes kMergeEntries entries at a time, lane l of it the tiles l, l + 64, ...
    // of each (consecutive lanes = consecutive addresses), four interleaved partial sums per lane, then a
    // shuffle tree over the lanes; the totals meet in LDS and are added to acc by one thread per entry
    // (one more latency, not one per group).  The order depends on n_tiles only, never on which tile
    // ran last.
    __threadfence();
    constexpr int kMergeEntries = 8, NWV = BLOCK / kWave, ITEMS = D + D * (D + 1) / 2;
    __shared__ double merged[ITEMS];
    const int w = threadIdx.x / kWave, l = threadIdx.x % kWave;
    for (int q0 = w * kMergeEntries; q0 < ITEMS; q0 += NWV * kMergeEntries) {
        const double *col[kMergeEntries];
#pragma unroll
        for (int e = 0; e < kMergeEntries; ++e) {
            const int q = (q0 + e < ITEMS) ? q0 + e : ITEMS - 1;       // the last group repeats an entry
            const int j = (q < D) ? q : D + pair_row(D, q - D) * D + pair_col(D, q - D);
            col[e] = rows + (int64_t)j * n_tiles;
        }
        double a[kMergeEntries][4];
#pragma unroll
        for (int e = 0; e < kMergeEntries; ++e)
#pragma unroll
            for (int i = 0; i < 4; ++i) a[e][i] = 0.0;
        uint32_t t = (uint32_t)l;
        for (; t + 3u * kWave < n_tiles; t += 4u * kWave) {
#pragma unroll
            for (int e = 0; e < kMergeEntries; ++e)
#pragma unroll
                for (int i = 0; i < 4; ++i) a[e][i] += col[e][t + (uint32_t)(i * kWave)];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (t + (uint32_t)(i * kWave) < n_tiles) {
#pragma unroll
                for (int e = 0; e < kMergeEntries; ++e) a[e][i] += col[e][t + (uint32_t)(i * kWave)];
            }
        }
#pragma unroll
        for (int e = 0; e < kMergeEntries; ++e) {
            double v = (a[e][0] + a[e][1]) + (a[e][2] + a[e][3]);
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
            if (l == 0 && q0 + e < ITEMS) merged[q0 + e] = v;
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < ITEMS; q += BLOCK) {
        const double v = merged[q];
        if (q < D) {
            acc[1 + q] += v;
        } else {   // mirror into both halves
            const int f = pair_row(D, q - D), g = pair_col(D, q - D);
            acc[1 + D + f * D + g] += v;
            if (g != f) acc[1 + D + g * D + f] += v;
        }
    }
    if (threadIdx.x == 0) {
        acc[0] += (double)n_roll * (double)H;
        *reinterpret_cast<uint32_t *>(acc + cov_sums(D)) = 0u;   // ready for the next pass
    }
}

// What a rollout launch of the ARS pipeline carries besides its rollouts (both optional):
//  * a progress flag: workgroup 0 stores flag_value to host-visible memory when it starts, i.e.
//    "everything enqueued on this stream before this launch has completed".  The host paces
//    itself on it, so the critical stream carries no event-record packets (measured: one costs
//    ~4 us between two kernels);
//  * the covariance pass over the PREVIOUS iteration's trajectories, run by extra workgroups
//    behind the rollout workgroups of the same grid: no second queue, no cross-queue events
//    (measured: a concurrent kernel on another queue costs the rollout launch ~5 us whatever
//    its size).  Those workgroups finish long before the rollouts do.
struct SideJob {
    uint32_t *flag;
    uint32_t flag_value;
    uint32_t first_cov_block;   // = number of rollout workgroups; UINT32_MAX: no covariance pass
    uint32_t cov_nbx;           // covariance tiles along the rollout axis
    uint32_t cov_tiles;         // covariance tiles in all
    int32_t cov_tchunk;         // steps per covariance tile
    int32_t cov_nap;            // s_sleep rounds per two steps of a split tile (load pacing)
    int32_t cov_H;
    int64_t cov_rolls;
    const double *cov_traj;
    double *cov_acc;
};

template <int D, int BLOCK>
__device__ __forceinline__ void side_cov_tile(const SideJob &sj)
{
    const uint32_t b = blockIdx.x - sj.first_cov_block;
    const uint32_t bx = b % sj.cov_nbx, by = b / sj.cov_nbx;
    const int32_t t0 = (int32_t)by * sj.cov_tchunk;
    moments_tile<D, BLOCK>(sj.cov_rolls, sj.cov_H, sj.cov_traj, sj.cov_acc, bx, t0,
                           min(sj.cov_H, t0 + sj.cov_tchunk), b, sj.cov_tiles, sj.cov_nap);
}

__device__ __forceinline__ void side_flag(const SideJob &sj)
{
    if (sj.flag && blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(sj.flag, sj.flag_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

const SideJob kNoSide{nullptr, 0u, UINT32_MAX, 1u, 0u, 0, 0, 0, 0, nullptr, nullptr};

// Attach a covariance pass over (cov_traj, cov_rolls, cov_H) to a launch of `roll_blocks` rollout
// workgroups of `block` threads; returns the number of extra workgroups.
unsigned side_attach_cov(SideJob &sj, unsigned roll_blocks, int block, int sj_D)
{
    sj.first_cov_block = roll_blocks;
    if (!sj.cov_traj || sj.cov_rolls <= 0 || sj.cov_H <= 0) {
        sj.first_cov_block = UINT32_MAX;
        return 0;
    }
    const sw_launch::CovTiling t = sw_launch::cov_tiling(sj.cov_rolls, sj.cov_H, block, sj_D, true);
    sj.cov_nbx = t.nbx;
    sj.cov_tchunk = t.tchunk;
    sj.cov_tiles = t.nbx * t.ny;
    static const char *nap_env = getenv("SWIMMER_COV_NAP");   // measurement knob
    sj.cov_nap = nap_env ? atoi(nap_env) : 0;
    return sj.cov_tiles;
}

// One launch of a segment-per-lane rollout kernel: the plan's rollout workgroups and, behind them, the covariance
// workgroups of the pass that rides along (side; may be null).
template <class Kernel>
void launch_segment_per_lane(Kernel *kernel, const sw_params *p, const sw_launch::RolloutPlan &plan, int64_t n_roll,
                             int32_t H, const sw_launch::RolloutArgs &a, hipStream_t stream,
                             const sw_launch::SideWork *side)
{
    SideJob sj = kNoSide;
    if (side) {
        sj.flag = side->flag;
        sj.flag_value = side->flag_value;
        sj.cov_traj = side->cov_traj;
        sj.cov_acc = side->cov_acc;
        sj.cov_rolls = side->cov_rolls;
        sj.cov_H = side->cov_H;
    }
    unsigned grid = plan.rollout_blocks;
    grid += side_attach_cov(sj, grid, plan.block, 2 * p->n + 2);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(plan.block), 0, stream, make_consts(p), n_roll, H, a.policies,
                       a.deltas, a.dir_begin, a.nu, a.mean, a.inv_std, a.state0, a.returns, a.traj, a.final_state,
                       a.moments, a.status, sj);
}

// The same for the form's ARS gate kernel, which carries no side job.
template <class Kernel>
void launch_gate_segment_per_lane(Kernel *kernel, const sw_params *sim, const sw_launch::RolloutPlan &plan,
                                  int64_t n_roll, int32_t H, const sw_launch::RolloutArgs &a, double gate_thr,
                                  int32_t *admit, hipStream_t stream)
{
    hipLaunchKernelGGL(kernel, dim3(plan.rollout_blocks), dim3(plan.block), 0, stream, make_consts(sim), n_roll, H,
                       a.policies, a.deltas, a.dir_begin, a.nu, a.mean, a.inv_std, gate_thr, admit, a.returns,
                       a.status, kNoSide);
}

}  // namespace
