// swimmer_cacla_learner.h -- the CACLA learner on the swimmer (cacla/cacla_agent.py:135-199), ONE WAVE PER AGENT: what
// cacla_kernel<N, TRAIN> (swimmer_cacla.hip) and cacla::gated_kernel<N, ENSEMBLE> (swimmer_cacla_gated.h, instantiated
// by swimmer_cacla_safe.hip and swimmer_cacla_ensemble.hip) run.  The kernels call the pieces below in the same order,
// so an ungated agent of sw_cacla_safe_run_f64 or sw_cacla_safe_ensemble_run_f64 has the bits of
// sw_cacla_run_f64(train = 1) by construction (tests/test_cacla_safe_gpu.py and tests/test_cacla_ensemble_gpu.py hold
// them to it at every n).
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
// t & 63 with v_readlane.
//
// Free functions over arrays that stay plain locals of the kernel, on purpose: a struct that owns W1, b1, W2 as
// members costs 26 .. 78 more registers per lane at n >= 6 (the compiler stops keeping the weights where it does now).
// Adding a step's noise to the actors' outputs stays a line of each kernel for the same reason: as a function here it
// costs the single-simulator gated kernel at n = 8 four registers, one allocation granule.  The run loop is a
// __global__ template for the same reason again: as a __device__ __forceinline__ function behind two thin kernels, its
// arguments by reference or by value, all 14 gated kernels change -- 26 .. 32 more AGPRs at n = 6, 7, 8 (one simulator,
// n = 8: 134 -> 162), 219 -> 242 VGPRs with one simulator at n = 5, 255 VGPRs + 2 AGPRs with an ensemble at n = 5, up to
// 160 more instructions.
#pragma once
#include "swimmer_launch.h"

namespace {
namespace cacla {

constexpr int kHid = SW_CACLA_HIDDEN;

template <int N> struct Shape {
    static constexpr int D = 2 * N + 2, M = N - 1;
    static constexpr int UPL = (kHid * N <= kWave) ? 1 : 2;   // hidden units per lane
    static constexpr int LPN = kHid / UPL;                    // lanes per network
    static constexpr int NETD = SW_CACLA_NET_DOUBLES(N);
    static_assert(LPN * N <= kWave && kHid % UPL == 0, "an agent's networks must fit one wave");
};

// Which hidden units a lane holds: units j0 .. j0 + UPL - 1 of network `net`.
struct Place {
    int lane, net, j0;
    bool valid;   // false: a lane behind the last network; it shadows the critic's unit 0 and stores nothing
};

template <int N> __device__ __forceinline__ Place place_of(int lane)
{
    using S = Shape<N>;
    const bool valid = lane < S::LPN * N;
    return Place{lane, valid ? lane / S::LPN : N - 1, valid ? (lane % S::LPN) * S::UPL : 0, valid};
}

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

// wn: the lane's network, SW_CACLA_NET_DOUBLES(N) doubles: W1 [12][d], b1 [12], W2 [12], b2
template <int N>
__device__ __forceinline__ void load_weights(const double *wn, int j0, double (&W1)[Shape<N>::UPL][Shape<N>::D],
                                             double (&b1)[Shape<N>::UPL], double (&W2)[Shape<N>::UPL], double &b2)
{
    constexpr int D = Shape<N>::D, UPL = Shape<N>::UPL;
#pragma unroll
    for (int u = 0; u < UPL; ++u) {
#pragma unroll
        for (int i = 0; i < D; ++i) W1[u][i] = wn[(j0 + u) * D + i];
        b1[u] = wn[kHid * D + j0 + u];
        W2[u] = wn[kHid * D + kHid + j0 + u];
    }
    b2 = wn[kHid * D + 2 * kHid];
}

template <int N>
__device__ __forceinline__ void store_weights(double *wn, int j0, const double (&W1)[Shape<N>::UPL][Shape<N>::D],
                                              const double (&b1)[Shape<N>::UPL], const double (&W2)[Shape<N>::UPL],
                                              double b2)
{
    constexpr int D = Shape<N>::D, UPL = Shape<N>::UPL;
#pragma unroll
    for (int u = 0; u < UPL; ++u) {
#pragma unroll
        for (int i = 0; i < D; ++i) wn[(j0 + u) * D + i] = W1[u][i];
        wn[kHid * D + j0 + u] = b1[u];
        wn[kHid * D + kHid + j0 + u] = W2[u];
    }
    if (j0 == 0) wn[kHid * D + 2 * kHid] = b2;
}

// sp: the agent's state, the observation's order: Gdot_x, Gdot_y, theta_1, thetadot_1, ...
template <int N>
__device__ __forceinline__ void load_state(const double *sp, double &gdx, double &gdy, double (&th)[N],
                                           double (&thd)[N])
{
    gdx = sp[0];
    gdy = sp[1];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        th[i] = sp[2 + 2 * i];
        thd[i] = sp[3 + 2 * i];
    }
}

template <int N>
__device__ __forceinline__ void observe(double gdx, double gdy, const double (&th)[N], const double (&thd)[N],
                                        double (&x)[Shape<N>::D])
{
    x[0] = gdx;
    x[1] = gdy;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        x[2 + 2 * i] = th[i];
        x[3 + 2 * i] = thd[i];
    }
}

// Stores the state; false when an entry is not finite (SW_STATUS_NONFINITE).  `&`, not `&&`: no branches between the
// stores.
template <int N>
__device__ __forceinline__ bool store_state(double *sp, double gdx, double gdy, const double (&th)[N],
                                            const double (&thd)[N])
{
    sp[0] = gdx;
    sp[1] = gdy;
    bool fin = isfinite(gdx) & isfinite(gdy);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        sp[2 + 2 * i] = th[i];
        sp[3 + 2 * i] = thd[i];
        fin = fin & isfinite(th[i]) & isfinite(thd[i]);
    }
    return fin;
}

// This lane's step of the 64-step block that starts at t0: its n - 1 noise values (0 behind the run's end).
template <int N>
__device__ __forceinline__ void load_noise(const double *np, int32_t n_iter, int32_t t0, int lane,
                                           double (&dst)[Shape<N>::M])
{
    constexpr int M = Shape<N>::M;
    const int64_t t = (int64_t)t0 + lane;
#pragma unroll
    for (int i = 0; i < M; ++i) dst[i] = (t < n_iter) ? np[t * M + i] : 0.0;
}

// A hidden unit before the relu: W1[j, :] . x + b1[j], even and odd entries in two chains.
template <int D> __device__ __forceinline__ double unit_input(const double (&w)[D], double b, const double (&x)[D])
{
    double z0 = b, z1 = w[1] * x[1];
    z0 = __builtin_fma(w[0], x[0], z0);
#pragma unroll
    for (int i = 2; i < D; i += 2) {
        z0 = __builtin_fma(w[i], x[i], z0);
        z1 = __builtin_fma(w[i + 1], x[i + 1], z1);
    }
    return z0 + z1;
}

// Forward of every network at x; prod: kWave * UPL doubles of LDS (lanes behind the last network write their own,
// unread slots).  Leaves this lane's h and relu mask for the update, and out = the actors' outputs, then V(x):
// wave-uniform.  relu as torch's: NaN passes (z <= 0 is false), and so does its gradient.
template <int N>
__device__ __forceinline__ void forward(double *prod, const Place &pl, const double (&W1)[Shape<N>::UPL][Shape<N>::D],
                                        const double (&b1)[Shape<N>::UPL], const double (&W2)[Shape<N>::UPL],
                                        double b2, const double (&x)[Shape<N>::D], double (&h)[Shape<N>::UPL],
                                        bool (&off)[Shape<N>::UPL], double (&out)[N])
{
    constexpr int UPL = Shape<N>::UPL, LPN = Shape<N>::LPN;
#pragma unroll
    for (int u = 0; u < UPL; ++u) {
        const double z = unit_input(W1[u], b1[u], x);
        off[u] = z <= 0.0;
        h[u] = off[u] ? 0.0 : z;
        prod[pl.lane * UPL + u] = W2[u] * h[u];
    }
    __syncthreads();
    const double own = __dadd_rn(sum_hidden(&prod[pl.net * kHid]), b2);
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = lane_value(own, i * LPN);
}

// The update behind a step from x (forward: h, off, out) with `act` to the state (gdx, gdy, th, thd), reward rew:
// V(s') with the weights from before the update (cacla_agent.py:186), the temporal difference, then this lane's
// network: the critic steps by alpha td, actor i by alpha (action_i - FA_act_i) if td > 0 (counted in n_upd).
template <int N>
__device__ __forceinline__ void learn(double *prod, const Place &pl, double (&W1)[Shape<N>::UPL][Shape<N>::D],
                                      double (&b1)[Shape<N>::UPL], double (&W2)[Shape<N>::UPL], double &b2,
                                      double gdx, double gdy, const double (&th)[N], const double (&thd)[N],
                                      const double (&x)[Shape<N>::D], const double (&h)[Shape<N>::UPL],
                                      const bool (&off)[Shape<N>::UPL], const double (&out)[N],
                                      const double (&act)[Shape<N>::M], double rew, double gam, double alp,
                                      int32_t &n_upd)
{
    constexpr int D = Shape<N>::D, M = Shape<N>::M, UPL = Shape<N>::UPL, LPN = Shape<N>::LPN;
    double xn[D];
    observe<N>(gdx, gdy, th, thd, xn);
#pragma unroll
    for (int u = 0; u < UPL; ++u) {
        const double z = unit_input(W1[u], b1[u], xn);
        prod[pl.lane * UPL + u] = W2[u] * ((z <= 0.0) ? 0.0 : z);
    }
    __syncthreads();
    const double v_new = lane_value(__dadd_rn(sum_hidden(&prod[pl.net * kHid]), b2), (N - 1) * LPN);
    const double td = __dadd_rn(__dadd_rn(rew, __dmul_rn(gam, v_new)), -out[N - 1]);
    const bool better = td > 0.0;            // false for NaN: no actor update, as the reference
    n_upd += better ? 1 : 0;
    double st = __dmul_rn(alp, td);
    bool upd = true;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const double sa = __dmul_rn(alp, __dadd_rn(act[i], -out[i]));
        st = (pl.net == i) ? sa : st;
        upd = (pl.net == i) ? better : upd;
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

}  // namespace cacla
}  // namespace
