// swimmer_cov.hip -- the standalone covariance pass (sw_traj_moments_f64, and the flush of a pass the ARS pipeline
// still owes) and the tiling of every pass; the tile itself is swimmer_cov.h.
#include "swimmer_cov.h"

using namespace sw_launch;

namespace {

constexpr int kMomTChunk = 32;  // steps per 256-thread tile (8 measured slower: less work per workgroup)
constexpr uint32_t kCovMaxTiles = 4096;   // tiles per pass: bounds the fixed-order merge

// standalone covariance pass: 1-D grid of nbx * ny tiles of BLOCK rollouts x tchunk steps
template <int D, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
traj_moments_kernel(int64_t n_roll, int32_t H, const double *__restrict__ traj,
                    double *__restrict__ acc, uint32_t nbx, int32_t tchunk)
{
    const uint32_t bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
    const int32_t t0 = (int32_t)by * tchunk;
    moments_tile<D, BLOCK>(n_roll, H, traj, acc, bx, t0, min(H, t0 + tchunk), blockIdx.x, gridDim.x);
}

}  // namespace

namespace sw_launch __attribute__((visibility("hidden"))) {

CovTiling cov_tiling(int64_t n_roll, int32_t H, int block, int D, bool riding)
{
    CovTiling t;
    const int cols = cov_split(D, block) ? kWave : block;   // rollouts per tile
    t.nbx = (uint32_t)((n_roll + cols - 1) / cols);
    // steps per tile: long tiles for the one-wave workgroups of the quad kernel's launches -- a tile
    // ends with a cross-lane reduction of all its accumulators, and once a batch puts a wave on
    // every SIMD those epilogues are the rollouts' time (2048 directions on one GPU, n = 3: launch
    // 0.2798 ms with 64 steps per tile, 0.2663 with 128, 0.384 with 32; no difference at 512
    // directions; profiles/r02_f_cov_tile_sweep.log)
    int32_t base = (block >= kMomBlock) ? (cov_split(D, block) ? 4 * kMomTChunk : kMomTChunk) : 128;
    if (!riding) {
        // alone on the chip the pass is fastest with ~one workgroup per CU for the split tiles, one per two
        // CUs for the wide ones -- fewer leave CUs idle, more lengthen the merge (0.06 us per tile):
        // profiles/r03_p_cov_tchunk_sweep.log
        const int64_t target = cov_split(D, block) ? 256 : 128;
        const int64_t want = ((int64_t)H * t.nbx + target - 1) / target;
        base = (int32_t)(want < 8 ? 8 : (want > H ? H : want));
    }
    static const char *env = getenv("SWIMMER_COV_TCHUNK");   // measurement knob
    if (env && atoi(env) > 0) base = atoi(env);
    const uint32_t ny_max = (uint32_t)((H + base - 1) / base);
    const uint32_t cap = kCovMaxTiles / t.nbx > 0 ? kCovMaxTiles / t.nbx : 1u;
    const uint32_t ny = ny_max < cap ? ny_max : cap;
    t.tchunk = (int32_t)((H + (int32_t)ny - 1) / (int32_t)ny);
    t.ny = (uint32_t)((H + t.tchunk - 1) / t.tchunk);
    return t;
}

// One covariance pass with workgroups of `block` (64, 128 or 256) threads.  The pipeline runs the pass
// it still owes with owed_cov_block() of the rollout launch that left it, so a flushed
// pass sums in exactly the order the ride-along pass would have (bit-identical resume).
int launch_traj_moments(const sw_params *p, int64_t n_roll, int32_t H, const double *traj,
                        double *acc, int block, bool riding, void *stream)
{
    if (n_roll < 0 || H < 0) return SW_ERR_SIZE;
    if (n_roll == 0 || H == 0) return SW_OK;
    if (!traj || !acc) return SW_ERR_NULL;
    const CovTiling t = cov_tiling(n_roll, H, block, 2 * p->n + 2, riding);
    auto launch = [&](auto *kernel, int threads) {
        hipLaunchKernelGGL(kernel, dim3(t.nbx * t.ny), dim3(threads), 0, (hipStream_t)stream, n_roll, H, traj, acc,
                           t.nbx, t.tchunk);
    };
    if (block == kOctBlock) {   // owed by a mirror-quad launch (n = 3 only)
        if (p->n != 3) return SW_ERR_SIZE;
        launch(traj_moments_kernel<8, kOctBlock>, kOctBlock);
        return launch_status();
    }
    const bool known_n = with_n<2, 8>(p->n, [&](auto N, auto ONE_WAVE) {
        constexpr int kBlock = ONE_WAVE.value ? kRollBlock : kMomBlock;
        launch(traj_moments_kernel<2 * N.value + 2, kBlock>, kBlock);
    }, block == kRollBlock);
    return known_n ? launch_status() : SW_ERR_SEGMENTS;
}

}  // namespace sw_launch

extern "C" {

int64_t sw_cov_acc_doubles(const sw_params *p, int64_t n_roll, int32_t H)
{
    if (validate_params(p) != SW_OK || n_roll < 0 || H < 0) return -1;   // pure host arithmetic
    const int d = 2 * p->n + 2;
    int64_t tiles = 0;
    if (n_roll > 0 && H > 0) {
        // every pass the batch can be given: riding or standalone, owed by a launch of any form
        // (sw_traj_moments_f64's standalone pass has the lane form's block)
        for (int riding = 0; riding < 2; ++riding)
            for (Form f : kForms) {
                const CovTiling t = cov_tiling(n_roll, H, owed_cov_block(f), d, riding != 0);
                const int64_t n = (int64_t)t.nbx * t.ny;
                tiles = n > tiles ? n : tiles;
            }
    }
    return cov_sums(d) + 1 + tiles * (d + d * d);
}

int sw_traj_moments_f64(const sw_params *p, int64_t n_roll, int32_t H, const double *traj,
                        double *acc, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    return launch_traj_moments(p, n_roll, H, traj, acc, kMomBlock, false, stream);
}

}  // extern "C"
