// swimmer_launch.h -- what the kernel families of libswimmer_hip.so share (internal; the C ABI is
// include/swimmer_hip.h): constants, tuning knobs, argument checks, the run-time-to-template dispatch, the rollout
// plan, and the four tables of launch functions -- one per kernel form -- that cross the files.
//
// All arithmetic is fp64 on the vector ALUs; there is no MFMA (the largest contraction on this
// path is 8x8) and no LDS in the hot loops (neighbour data moves by DPP).  One source file per kernel family, each
// with its kernels, their private device helpers and the host function that launches them (swimmer_kernels.hip
// includes the families' files into the one translation unit their code depends on; its header says why):
//
//   swimmer_step.hip
//   step_kernel<N,TWIN,NT>     one physics step, SoA in / SoA out, one env per lane; HBM-bound
//                              at large n_env (algorithmic traffic 16 (2n+2) + 8 (n-1) + 8 bytes
//                              per env-step); NT = nontemporal accesses for streaming batches.
//                              A two-envs-per-lane variant with 16-byte accesses measured SLOWER
//                              (4.87 vs 5.62 TB/s: 90 VGPRs, fewer loads in flight) and was dropped.
//   accel_kernel<N,TWIN>       accelerations only
//   step_residual*_kernel      the estimator's objective, one parameter set or a population
//   step_residual_sets_kernel<N>  the population objective for MANY ESTIMATORS in one launch (sw_step_residual_sets_f64):
//                              candidate j scores on transition set cand_set[j]; blocks are counted from the set's
//                              first column, so every partial has step_residual_kernel's bits on the set alone
//   step_residual_normal_sets_kernel<N,NP>  the least-squares refinement's r.r (NP = 1) or r.r | J^T J | J^T r (NP = 7,
//                              central differences in registers) per transition set, fixed-order sums
//                              (sw_step_residual_normal_sets_f64); residual_set_rows_sum_kernel adds both kernels'
//                              per-block rows in residual_rows_sum_kernel's order
//   env1_kernel                one swimmer handed over in host memory (sw_env1)
//   swimmer_rollout_n3.hip
//   rollout_oct3_kernel        n = 3, H steps in one launch, one segment per lane WITH LANE ROLES: two
//                              mirror quads per rollout (sine / cosine, Gdot_x / Gdot_y;
//                              swimmer_oct3.h): the latency form, instruction-issue bound; up to
//                              8192 rollouts (one wave per SIMD)
//   rollout_octp3_kernel       the same with capture AND V2 moments in the packed record form: one trajectory store
//                              and one moment pair per step (swimmer_rollout_octp3.inc); bit-identical outputs;
//   rollout_octl3_kernel       the packed record form with a leaner step (the same body, SW_OCTP_LEAN 1): store
//                              offsets from loop-invariant SGPRs, range test on vcc (SW_FLAG_CAPTURE_LEAN_V1)
//   rollout_octs3_kernel       the lean mode with the neighbour's matrix entry (SW_OCTP_NEXT_E 1): Q(i+1, i+2) comes
//                              from lane i+1 through DPP, three f64 instructions fewer per step; the default of such
//                              a launch.  SW_FLAG_CAPTURE_LEAN_V1 keeps it on rollout_octl3_kernel,
//                              SW_FLAG_CAPTURE_PACKED_V1 on rollout_octp3_kernel,
//                              SW_FLAG_CAPTURE_SPLIT on rollout_oct3_kernel<.., true, true>
//   rollout_quad3_kernel       n = 3, one DPP quad per rollout (swimmer_quad3.h): 8193 .. 16384 rollouts
//   swimmer_rollout_row.hip
//   rollout_row_kernel<N>      n = 4..8, one segment per lane, one rollout per 16-lane DPP row
//                              (swimmer_row.h)
//   swimmer_rollout_lane.hip
//   rollout_kernel<N,ARS,TWIN> any n, ONE ROLLOUT PER LANE: the throughput form for batches that
//                              fill the chip, and the only form of the twin model
//   (each rollout file also holds its form's ARS gate and safe-exploration kernels)
//   ars_multi_oct3_kernel<MOM>, ars_multi_quad3_kernel<MOM>, ars_multi_row_kernel<N,MOM>,
//   ars_multi_lane_kernel<N,TWIN>  (one per form, in the form's file)
//                              sw_ars_rollouts_multi_f64: the ARS rollouts of MANY AGENTS in one launch, grid
//                              (workgroups of one agent, n_agent).  Each is its form's body (the .inc file) behind
//                              swimmer_rollout_multi.inc, which points policy, deltas, mean, inv_std and the outputs
//                              at the slices of agent blockIdx.y: per rollout the arithmetic of the
//                              single-agent kernel without capture, hot loops pinned by the body's SW_PIN_LOOP with
//                              pads of their own (*_multi_loop_pad below)
//   ars_gate_multi_{oct3,quad3,row,lane}_kernel, ars_counted_{oct3,quad3,row,lane}_kernel  (in the form's file)
//                              sw_ars_gate_multi_f64 / sw_ars_rollouts_multi_counted_f64: the safe half of a batch of
//                              agents.  The gate form takes every agent's simulator constants and threshold from device
//                              arrays (the view derives C with sw::consts_of), the counted form every agent's number
//                              of rollouts; both are the form's body behind swimmer_rollout_multi.inc
//   ars_gate_ens_{oct3,quad3,row,lane}_kernel  (in the form's file)
//                              the member launch of sw_ars_gate_ensemble_f64: the gate body behind the same view with
//                              SW_MULTI_ENSEMBLE 1, grid (workgroups of one agent, n_agent * n_sim): member (a, e) runs
//                              agent a's policy and deltas in simulator sim[a][e] and writes its own slices;
//                              ars_gate_fold_kernel (swimmer_abi.hip) then folds the members into admit / worst / status
//   swimmer_rollout_safe_multi.hip
//   safe_ars_multi_oct3_kernel<COST,VIOL>, safe_ars_multi_lane_kernel<N>
//                              sw_safe_ars_rollouts_multi_f64: the ARS exploration rollouts of MANY AGENTS with the
//                              per-step simulator gate (Safe_ARS.rollout) or without it (Basic_ARS.rollout), agent by
//                              agent: the safe-exploration bodies (swimmer_rollout_safe_oct3.inc, _lane.inc, shared with
//                              safe_rollout_oct3_kernel / safe_rollout_kernel) behind swimmer_rollout_safe_multi.inc;
//                              per step one cost value per rollout instead of a trajectory
//   swimmer_safe_ars_ensemble.hip (a translation unit of its own)
//   safe_ars_ensemble_kernel<N>  sw_safe_ars_rollouts_ensemble_f64: the lane body of the kernels above
//                              (swimmer_rollout_safe_lane.inc with SW_SAFE_ENSEMBLE 1) with a rollout in a GROUP of
//                              2^k >= n_member lanes, lane j with the constants of member j % n_member of the agent's
//                              simulator ensemble in VGPRs: the look-ahead of every member in the same instructions,
//                              the gate a wave ballot cut to the group, which also names the refusing members; the
//                              worst admitted member cost a per-lane running maximum, reduced once behind the loop
//   swimmer_update.hip
//   ars_update_kernel          sigma_R, policy step, V2 statistics merge; pure latency between
//                              two rollout launches: one round of loads, then LDS only
//   ars_update_multi_kernel    the same body (swimmer_update.inc) for many agents, grid (m*d + 1, n_agent)
//   ars_update_counted_kernel  the same with every agent's direction count read on the device (0: agent untouched)
//   ars_pack_admitted_kernel   admit flags -> count, ascending order, packed deltas; one workgroup per agent
//   swimmer_cov.hip, swimmer_cov.h
//   traj_moments_kernel<D>     full first/second moments of a trajectory buffer; HBM-bound; its tile code
//                              (swimmer_cov.h) also rides along in the segment-per-lane rollout launches (SideJob)
//   swimmer_cacla_learner.h     the CACLA learner of the three files below: the layout of an agent's networks over its
//                              wave, weight / state / noise loads and stores, forward<N> and learn<N>
//   swimmer_cacla.hip (a translation unit of its own)
//   cacla_kernel<N,TRAIN>      sw_cacla_run_f64: CACLA training runs of many independent agents, n_iter sequential
//                              steps in one launch, ONE WAVE PER AGENT: the agent's n two-layer networks in registers
//                              (a hidden unit per lane, two from n = 6), the physics redundantly in every lane, the
//                              n + 1 network outputs of a step summed through LDS in a fixed order and handed out
//                              with v_readlane; instruction-issue bound like the latency forms
//   swimmer_cacla_gated.h      the gated run loop of the two files below, ONE kernel body: cacla::gated_kernel<N, ENSEMBLE>,
//                              with their argument check and launch (cacla::gated_run<ENSEMBLE>)
//   swimmer_cacla_safe.hip (a translation unit of its own)
//   cacla::gated_kernel<N, false>  sw_cacla_safe_run_f64: the same learner behind a per-step simulator gate, per agent
//                              gated or not: cacla_kernel's learner in its order (an ungated agent has its bits), plus the
//                              simulator's look-ahead step and the cost redundantly in every lane, the admit decision
//                              taken from the first lane into a scalar register, the real step and the update behind
//                              a uniform branch; reward entry and admit flag staged per lane, stored once per block
//   swimmer_cacla_ensemble.hip (a translation unit of its own)
//   cacla::gated_kernel<N, true>  sw_cacla_safe_ensemble_run_f64: the same run loop with the look-ahead in an
//                              ENSEMBLE of up to 64 simulators: lane L holds the constants of member L % n_member in
//                              VGPRs, so the same instructions look ahead in every member; the admit decision is a wave
//                              ballot over every lane's verdict; optionally the worst member cost per step (a wave
//                              maximum behind a uniform branch) and per-member refusal counts
//   swimmer_lqr.hip (a translation unit of its own)
//   lqr_cacla_kernel<NS,NA,MODE>  sw_lqr_cacla_run_f64: CACLA on LQR problems (plain, safe with a per-step or a fixed
//                              simulator threshold), ONE AGENT PER LANE: models, F, V and state in VGPRs, no LDS, no
//                              cross-lane traffic; agent-minor arrays, the noise loaded a block of steps ahead
//   swimmer_abi.hip
//   the rollout entry points and the native ARS iteration pipeline (sw_ars_pipeline_*: copy stream, progress
//   flag, 4-slot buffer ring; the covariance pass rides along in the next rollout launch)
// Which of the four rollout forms a launch takes, and with which grid, is decided in ONE place,
// plan_rollouts() (swimmer_abi.hip); run-time flags and n become template arguments through with_bools() /
// with_n<LO, HI>(), next to the kernels they name.
//
// Kernels and the types they take stay in unnamed namespaces (their mangled names are what the ISA tools, the
// placement test and the profiles key on), and so do the functions that launch them: what crosses the files is in
// namespace sw_launch below, with hidden visibility -- the library's dynamic symbols are the C ABI only -- and of the
// launch functions only ONE table of pointers per form (FormLaunchers), reached through launchers(plan.form).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <climits>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "../../include/swimmer_hip.h"
#include "swimmer_device.h"
#include "swimmer_twin.h"

// Where a rollout kernel's hot loop starts inside a 64-byte line of code.  A lone wave's issue rate depends on
// it: the same instructions, byte for byte, ran 0.2267 and 0.2346 ms per launch (n = 3) after an unrelated
// change elsewhere in the file had moved the loop by 16 bytes, and the one-step loops of the row kernel lose
// 4-11 % when their head is not 8-byte aligned (profiles/r03_p_ab_n3.log, r03_p_loop_pad_sweep_*.log).
// SW_PIN_LOOP aligns the code that follows to a line and puts PAD s_nops (4 bytes each) behind the boundary;
// the pads below are the best of a sweep over 0..7 on the GPU (scripts/ab_probe.sh over builds with
// -DSW_OCT_LOOP_PAD=k -DSW_QUAD_LOOP_PAD=k -DSW_ROW_LOOP_PAD=k).  Sweep again after changing what lies
// between a pin and its loop.
#define SW_PIN_LOOP(PAD) asm volatile(".p2align 6\n\t.fill %0, 4, 0xbf800000" ::"n"(PAD))
#ifndef SW_OCT_UNROLL
#define SW_OCT_UNROLL 8   // steps per trip of the mirror-quad kernel's main loop (4 or 8)
#endif
// mirror-quad kernel, by what the loop carries (trajectory capture, V2 moment sums): every instantiation is
// its own code, with its own best offset (profiles/r03_x_inst_sweep.log); -DSW_OCT_LOOP_PAD=k overrides all four
#ifdef SW_OCT_LOOP_PAD
constexpr int oct_loop_pad(bool, bool) { return SW_OCT_LOOP_PAD; }
#else
constexpr int oct_loop_pad(bool traj, bool mom) { return traj ? (mom ? 5 : 6) : (mom ? 6 : 2); }
#endif
// the packed-record form of the mirror-quad kernel (rollout_octp3_kernel): other code between pin and loop, a pad of
// its own.  Swept over all sixteen 4-byte offsets (profiles/r06_b_octp_pad_sweep.log, two passes): the even pads, which
// start the loop on an 8-byte boundary, ran 0.2164-0.2182 ms per launch, the odd ones 0.2176-0.2204; 2, 4 and 6 are
// the best three (0.2164-0.2167), 4 is pinned.  -DSW_OCTP_LOOP_PAD=k overrides it for a sweep
#ifndef SW_OCTP_LOOP_PAD
#define SW_OCTP_LOOP_PAD 4
#endif
constexpr int oct_packed_loop_pad() { return SW_OCTP_LOOP_PAD; }
// its lean mode (rollout_octl3_kernel): other instructions in the loop (5688 bytes), a pad of its own.  Swept over the
// eight even pads, the ones that start the loop on an 8-byte boundary (profiles/r08_b_octl_pad_sweep.log, two passes):
// 0.2093-0.2125 ms per launch; 2 and 10 (loop head at offset 0 and 32 of its line) are the best two in both passes
// (0.2093-0.2101), 2 is pinned.  -DSW_OCTL_LOOP_PAD=k overrides it for a sweep
#ifndef SW_OCTL_LOOP_PAD
#define SW_OCTL_LOOP_PAD 2
#endif
constexpr int oct_lean_loop_pad() { return SW_OCTL_LOOP_PAD; }
// the lean mode with the neighbour's matrix entry (rollout_octs3_kernel): other instructions in the loop again, a pad
// of its own.  Swept over the eight even pads with sixteen steps per trip (profiles/r13_b_octs_pad_sweep.log, two
// passes; the loop is 11288 bytes): 0.2015-0.2059 ms per launch; 2 and 10 (loop head at offset 0 and 32 of its line) are
// the best two in both passes (0.2015-0.2023), 2 is pinned.  -DSW_OCTS_LOOP_PAD=k overrides it for a sweep
#ifndef SW_OCTS_LOOP_PAD
#define SW_OCTS_LOOP_PAD 2
#endif
constexpr int oct_next_e_loop_pad() { return SW_OCTS_LOOP_PAD; }
// rollout_octs3_kernel alone: a main loop of sixteen steps per trip ahead of the eight-step one (eight more pinned
// SGPRs of store offsets).  Measured in the same sweep: 0.2016 against 0.2048 ms per launch with eight steps per trip
// (both at pad 2; that kernel's own repeats are 0.0008 apart), so it is on; 0 is the eight-step loop, for measurement.
// (A trip counter that counts down, two scalar instructions fewer per trip, gained 0.0013 ms on the eight-step loop
// and nothing on this one, 0.2019 against 0.2016: not kept.)
#ifndef SW_OCTS_TRIP16
#define SW_OCTS_TRIP16 1
#endif
#ifndef SW_QUAD_LOOP_PAD
#define SW_QUAD_LOOP_PAD 0
#endif
// row kernel, n = 4..8; swept with capture + moments for every n, and for the other three forms at n = 6;
// -DSW_ROW_LOOP_PAD=k overrides all of them for a sweep
#ifdef SW_ROW_LOOP_PAD
constexpr int row_loop_pad(int, bool, bool) { return SW_ROW_LOOP_PAD; }
#else
constexpr int row_loop_pad(int n, bool traj, bool mom)
{
    if (n == 6 && !(traj && mom)) return traj ? 6 : 4;
    return n == 4 ? 5 : n == 5 ? 0 : n == 6 ? 5 : n == 7 ? 6 : 1;
}
#endif

// The multi-agent kernels (ars_multi_*_kernel, sw_ars_rollouts_multi_f64) run their form's body behind another
// prologue, so the same pad leaves their loops elsewhere in the line: they have pads of their own.
//  * mirror-quad (n = 3, the form a batch of seeds runs in): SWEPT on the GPU over the eight pads that start the loop
//    on an 8-byte boundary (1, 3, .. 15; profiles/r05_multi_pad_sweep.log, S = 1 and 64 agents, two passes).  At the
//    pad that puts the V2 loop where its single-agent twin's sits (12: offset 28) the launch ran 205.0 us against the
//    twin's 198.3; at every odd pad 197.9-199.1.  V1: 188.2-190.1, best at 3 and 11.  Pad 11 for both: 188.3 (twin
//    188.6) and 198.2 (twin 198.3).
//  * quad and row: NOT swept.  Each pad puts the hot loop at the offset its single-agent twin (the form's ARS kernel
//    without capture, same n, same MOM) has in the same build -- scripts/multi_loop_offsets.py prints both -- where
//    the loops hold the same instructions (row) or differ by one scalar move (quad).
// -DSW_MULTI_LOOP_PAD=k overrides all of them for a sweep.
#ifdef SW_MULTI_LOOP_PAD
constexpr int oct_multi_loop_pad(bool) { return SW_MULTI_LOOP_PAD; }
constexpr int quad_multi_loop_pad(bool) { return SW_MULTI_LOOP_PAD; }
constexpr int row_multi_loop_pad(int, bool) { return SW_MULTI_LOOP_PAD; }
#else
constexpr int oct_multi_loop_pad(bool) { return 11; }
constexpr int quad_multi_loop_pad(bool) { return 3; }
constexpr int row_multi_loop_pad(int n, bool mom)
{
    return n == 4 ? (mom ? 1 : 3) : n == 5 ? (mom ? 11 : 15) : n == 6 ? (mom ? 11 : 13) : n == 7 ? (mom ? 10 : 1)
                                                                                                 : (mom ? 9 : 4);
}
#endif

// The multi-agent gate kernels (ars_gate_multi_*_kernel) and the counted multi-agent rollout kernels
// (ars_counted_*_kernel) of the safe batch have prologues of their own again.  Their pads are NOT swept: each puts the
// hot loop at the offset its single-agent twin has in the same build (the form's gate kernel, resp. the form's ARS
// kernel without capture, same n, same MOM); scripts/multi_loop_offsets.py prints both offsets for these pairs too.
// -DSW_SAFE_MULTI_LOOP_PAD=k overrides all of them.
#ifdef SW_SAFE_MULTI_LOOP_PAD
constexpr int oct_gate_multi_loop_pad() { return SW_SAFE_MULTI_LOOP_PAD; }
constexpr int quad_gate_multi_loop_pad() { return SW_SAFE_MULTI_LOOP_PAD; }
constexpr int row_gate_multi_loop_pad(int) { return SW_SAFE_MULTI_LOOP_PAD; }
constexpr int oct_counted_loop_pad(bool) { return SW_SAFE_MULTI_LOOP_PAD; }
constexpr int quad_counted_loop_pad(bool) { return SW_SAFE_MULTI_LOOP_PAD; }
constexpr int row_counted_loop_pad(int, bool) { return SW_SAFE_MULTI_LOOP_PAD; }
#else
constexpr int oct_gate_multi_loop_pad() { return 2; }
constexpr int quad_gate_multi_loop_pad() { return 0; }
constexpr int row_gate_multi_loop_pad(int n) { return n == 4 ? 10 : n == 5 ? 4 : n == 6 ? 12 : n == 7 ? 0 : 7; }
constexpr int oct_counted_loop_pad(bool mom) { return mom ? 12 : 11; }
constexpr int quad_counted_loop_pad(bool) { return 3; }
constexpr int row_counted_loop_pad(int n, bool mom)
{
    return n == 4 ? (mom ? 14 : 0) : n == 5 ? (mom ? 8 : 12) : n == 6 ? (mom ? 8 : 10) : n == 7 ? (mom ? 10 : 14)
                                                                                             : (mom ? 6 : 1);
}
#endif

// The member kernels of the ensemble gate (ars_gate_ens_*_kernel, sw_ars_gate_ensemble_f64) run the gate body behind
// the ensemble view, whose prologue divides blockIdx.y by the ensemble size: pads of their own once more.  NOT swept
// either: each puts the hot loop at the offset of the form's ars_gate_multi_*_kernel (scripts/multi_loop_offsets.py
// prints these pairs too).  -DSW_ENS_LOOP_PAD=k overrides all of them.
#ifdef SW_ENS_LOOP_PAD
constexpr int oct_gate_ens_loop_pad() { return SW_ENS_LOOP_PAD; }
constexpr int quad_gate_ens_loop_pad() { return SW_ENS_LOOP_PAD; }
constexpr int row_gate_ens_loop_pad(int) { return SW_ENS_LOOP_PAD; }
#else
constexpr int oct_gate_ens_loop_pad() { return 2; }
constexpr int quad_gate_ens_loop_pad() { return 0; }
constexpr int row_gate_ens_loop_pad(int n) { return n == 4 ? 10 : n == 5 ? 4 : n == 6 ? 12 : n == 7 ? 12 : 7; }
#endif

// steps per trip of the quad kernel's loop (measurement knob; 2 measured +5 ns per step)
#ifndef SW_QUAD_UNROLL
#define SW_QUAD_UNROLL 4
#endif
// Cache policy of the trajectory stores of the segment-per-lane kernels (gfx940+ encoding:
// 1 = sc0, 2 = nt, 16 = sc1).  sc1 = device-scope write-through: the 65 MB a launch stores do not
// pile up as dirty lines in the XCDs' L2s, so the write-back at the end of the kernel -- which sits
// on the critical path rollout -> update -- is short.  Same-box A/B (profiles/r02_d_ab_store_policy.log):
// plain 0.2564 ms per launch / 0.2675 ms per iteration, nt 0.2550 / 0.2658, sc0 0.2566 / 0.2673,
// sc1 0.2520 / 0.2628 (sc0 + sc1 and sc1 + nt the same as sc1).  (The lane kernel's stores in the
// saturated regime gain nothing from nontemporal stores: 4.58 vs 4.55 TB/s, scripts/saturated_probe.py.)
#ifndef SW_TRAJ_STORE_AUX
#define SW_TRAJ_STORE_AUX 16
#endif
// n = 3 rollouts: the mirror-quad kernel (swimmer_oct3.h) by default, or the quad kernel
#ifndef SW_N3_DEFAULT_OCT
#define SW_N3_DEFAULT_OCT true
#endif

namespace {

constexpr int kWave = 64;
constexpr int kStepBlock = 256;
constexpr int kRollBlock = 64;   // one wave per workgroup: every wave gets a SIMD to itself
constexpr int kOctBlock = 128;   // mirror-quad kernel: 8 rollouts per wave, 16 (= one V2 moment row) per workgroup
constexpr int kMomGroup = 16;    // rollouts per V2 moment row (same partition in every kernel)
constexpr int64_t kOctMaxRollouts = 8192;    // mirror-quad kernel (n = 3): one wave per SIMD up to here
constexpr int64_t kQuadMaxRollouts = 16384;  // above this every SIMD already has a wave
constexpr int64_t kRowMaxRollouts = 8192;    // row kernel (n >= 4): 4 rollouts per wave
constexpr int kRowBlock = 256;               // 16 rollouts = one V2 moment row per workgroup
constexpr int kUpdBlock = 256;        // update kernel: threads per workgroup up to kUpdWideFrom directions ...
constexpr int kUpdBlockWide = 1024;   // ... and beyond (a thread's share of the directions stays short)
constexpr int32_t kUpdWideFrom = 1025;
constexpr int kMomBlock = 256;        // standalone covariance pass: threads per workgroup
constexpr int64_t kStepStreamBytes = (int64_t)256 << 20;   // beyond the Infinity Cache: nontemporal accesses
constexpr int kPopGroup = 8;          // sw_step_residual_pop_f64: candidates per workgroup, ...
constexpr int64_t kPopMaxCandidates = (int64_t)65535 * kPopGroup;   // ... and at most 65535 groups (grid.y)
constexpr int64_t kSetsMax = 65535;   // sw_step_residual_normal_sets_f64: one grid row (grid.y) per transition set
constexpr double kHalfPi = 1.57079632679489661923;  // math.pi / 2 (remy_swimmer_env.py:65)
constexpr double kTwinStart = 0.001;                // SwimmerEnvironment.cpp:41

sw::Consts make_consts(const sw_params *p)
{
    return sw::consts_of(p->n, p->l_i, p->m_i, p->k, p->h, p->dir_x, p->dir_y);
}

sw::TwinConsts make_twin_consts(const sw_params *p)
{
    return sw::TwinConsts{p->l_i, p->m_i, p->k, p->h, p->dir_x, p->dir_y};
}

inline bool is_twin(const sw_params *p) { return (p->flags & SW_FLAG_MODEL_TWIN) != 0; }

// Argument check shared by the entry points and the internal launchers (touches no HIP state).
int validate_params(const sw_params *p)
{
    if (!p) return SW_ERR_NULL;
    if (p->n < 2 || p->n > SW_MAX_SEGMENTS) return SW_ERR_SEGMENTS;
    if (p->flags & ~(SW_FLAG_ROLLOUT_LANE | SW_FLAG_ROLLOUT_QUAD | SW_FLAG_MODEL_TWIN | SW_FLAG_CAPTURE_SPLIT |
                     SW_FLAG_CAPTURE_PACKED_V1 | SW_FLAG_CAPTURE_LEAN_V1))
        return SW_ERR_PARAM;
    if ((p->flags & SW_FLAG_CAPTURE_SPLIT) && (p->flags & SW_FLAG_CAPTURE_PACKED_V1)) return SW_ERR_PARAM;   // one or the other
    if ((p->flags & SW_FLAG_CAPTURE_LEAN_V1) && (p->flags & (SW_FLAG_CAPTURE_SPLIT | SW_FLAG_CAPTURE_PACKED_V1)))
        return SW_ERR_PARAM;   // at most one of the three
    if (!(p->l_i > 0.0) || !(p->m_i > 0.0) || !isfinite(p->l_i) || !isfinite(p->m_i) ||
        !isfinite(p->k) || !isfinite(p->h) || !isfinite(p->dir_x) || !isfinite(p->dir_y))
        return SW_ERR_PARAM;
    return SW_OK;
}

// First call of every PUBLIC entry point: drops, once, whatever error an earlier HIP call of this
// thread left behind (a failed call of the caller's, hipErrorNotReady from an event query, ...), so
// that launch_status() reports OUR launches and does not blame a stale error on them.  Internal
// launchers use validate_params(): clearing again in the middle of an entry point would discard
// the error of a launch the entry point itself made a moment earlier.
int check_params(const sw_params *p)
{
    (void)hipGetLastError();
    return validate_params(p);
}

int launch_status()
{
    return hipGetLastError() == hipSuccess ? SW_OK : SW_ERR_LAUNCH;
}

// The state cost of the safe-exploration entry points (SW_COST_*): a known kind, and for |obs[index]| an index inside
// the real model's observation.
int check_cost(const sw_params *real, int32_t cost_kind, int32_t cost_index)
{
    if (cost_kind != SW_COST_ABS_OBS && cost_kind != SW_COST_MAX_ABS_THETADOT) return SW_ERR_SIZE;
    if (cost_kind == SW_COST_ABS_OBS && (cost_index < 0 || cost_index >= 2 * real->n + 2)) return SW_ERR_SIZE;
    return SW_OK;
}

// ---- dispatch on the segment count -------------------------------------------------
// Run-time values to template arguments.  f is a generic lambda that takes them BY VALUE as
// std::integral_constant, so `N.value` / `TRAJ.value` are constant expressions inside it.
template <class F> void with_bools(F &&f) { f(); }
template <class F, class... Rest> void with_bools(F &&f, bool b, Rest... rest)
{
    if (b)
        with_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else
        with_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

// f(N, bools...) for n in the closed range LO..HI -- the only values a kernel is instantiated for;
// false (the caller's SW_ERR_SEGMENTS) when n is outside it.
template <int LO, int HI, class F, class... Bools> bool with_n(int n, F &&f, Bools... bools)
{
    if constexpr (LO > HI) {
        return false;
    } else {
        if (n != LO) return with_n<LO + 1, HI>(n, f, bools...);
        with_bools([&](auto... cs) { f(std::integral_constant<int, LO>{}, cs...); }, bools...);
        return true;
    }
}

// ------------------------------------------------------------------------------------
// The ARS simulator gate (sw_ars_gate_f64, ars_agent.py:146-157): direction i is admitted unless one of
// its two simulator returns is <= the threshold.  `x <= thr` is false for a NaN on either side, so a
// NaN return or a NaN threshold admits, as in the reference.  Rollouts 2i and 2i + 1 of a direction
// sit in one wave in every kernel form, XOR lanes apart: one ds_swizzle (bit-mask mode, XOR < 32)
// hands each owner lane its partner's return, the even rollout's owner stores the flag.  Every lane
// of the pair's owners must be active (both rollouts of a direction are valid or neither is).
template <int XOR>
__device__ __forceinline__ double swizzle_xor_f64(double v)
{
    static_assert(XOR > 0 && XOR < 32, "ds_swizzle bit-mask mode reaches lanes within 32");
    constexpr int kPattern = 0x1f | (XOR << 10);   // and_mask 0x1f, or_mask 0, xor_mask XOR
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_ds_swizzle(lo, kPattern);
    hi = __builtin_amdgcn_ds_swizzle(hi, kPattern);
    return __hiloint2double(hi, lo);
}

template <int XOR>
__device__ __forceinline__ void gate_store(double ret, int code, bool owner, int64_t r, double thr,
                                           double *__restrict__ returns, int32_t *__restrict__ status,
                                           int32_t *__restrict__ admit)
{
    const double partner = swizzle_xor_f64<XOR>(ret);
    if (owner) {
        if (returns) returns[r] = ret;
        if (status) status[r] = code;
        if ((r & 1) == 0) admit[r >> 1] = (!(ret <= thr) && !(partner <= thr)) ? 1 : 0;
    }
}

// A value every lane of the wave holds, moved to scalar registers (the per-agent constants of the safe batch's gate
// are derived in the kernel from a device array: the bodies expect them where kernel arguments live).
__device__ __forceinline__ double uniform_f64(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

__device__ __forceinline__ sw::Consts uniform_consts(const sw::Consts &c)
{
    return sw::Consts{uniform_f64(c.l),       uniform_f64(c.h),       uniform_f64(c.dirx),
                      uniform_f64(c.diry),    uniform_f64(c.kl_nm),   uniform_f64(c.h_kl_nm),
                      uniform_f64(c.six_k_m), uniform_f64(c.kl_m),    uniform_f64(c.c12)};
}

// the parameter rule of validate_params for a parameter set read on the device
__device__ __forceinline__ bool sim_params_ok(double l, double m, double k)
{
    return l > 0.0 && m > 0.0 && isfinite(l) && isfinite(m) && isfinite(k);
}

// The state costs of the safe-exploration kernels (include/swimmer_hip.h SW_COST_*), one rollout per lane:
// |obs[index]|, or max_i |thetadot_i| with np.max's NaN rule.
template <int N>
__device__ __forceinline__ double safe_cost(int32_t kind, int32_t index, double gdx, double gdy,
                                            const double (&th)[N], const double (&thd)[N])
{
    if (kind == SW_COST_MAX_ABS_THETADOT) {
        double c = fabs(thd[0]);
#pragma unroll
        for (int i = 1; i < N; ++i) c = fmax(c, fabs(thd[i]));   // np.max: NaN handled by the caller's <= test
        bool nan = false;
#pragma unroll
        for (int i = 0; i < N; ++i) nan = nan || (thd[i] != thd[i]);
        return nan ? __builtin_nan("") : c;                      // np.max propagates NaN, fmax would drop it
    }
    double v = (index == 0) ? gdx : gdy;                         // |obs[index]|, obs = [Gdx, Gdy, th_1, thd_1, ...]
#pragma unroll
    for (int i = 0; i < N; ++i) {
        v = (index == 2 + 2 * i) ? th[i] : v;
        v = (index == 3 + 2 * i) ? thd[i] : v;
    }
    return fabs(v);
}

// mirror-quad safe-exploration kernels: a value committed where the gate is open
__device__ __forceinline__ double oct_sel(bool take, double a, double b) { return take ? a : b; }

// This lane's pre-combined policy row V_i = c12 (W_{i-1} - W_i), W = (P +- nu delta) diag(inv_std)
// (ars_agent.py:141-142, environment.py:32-34; u_{-1} = u_{n-1} = 0: free ends), and
// nbias = -V_i . mean.  cols[j]: the observation column of entry j (the quad kernel keeps its
// row in rotated order).  Branch-free on purpose: every lane loads both neighbouring rows with a
// clamped row index and SELECTS afterwards, so all 4 D + 2 D loads are in flight together and the
// launch pays one memory latency instead of ~40 serial ones (measured: the prologue was most of
// the ~6 us fixed cost of a rollout launch).
template <int D, int M, bool ARS>
__device__ __forceinline__ void load_policy_row(const double *__restrict__ pl,
                                                const double *__restrict__ dl, double sgn, double nu,
                                                const double *__restrict__ mean,
                                                const double *__restrict__ inv_std, double c12,
                                                int seg, const int (&cols)[D], double (&V)[D],
                                                double &nbias)
{
    const int a_up = (seg >= 1) ? seg - 1 : 0, a_dn = (seg <= M - 1) ? seg : M - 1;
    double pu[D], pd[D], du[D], dd[D], is[D], mn[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        pu[j] = pl[a_up * D + cols[j]];
        pd[j] = pl[a_dn * D + cols[j]];
    }
    if (ARS) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            du[j] = dl[a_up * D + cols[j]];
            dd[j] = dl[a_dn * D + cols[j]];
        }
    }
    if (inv_std) {   // uniform
#pragma unroll
        for (int j = 0; j < D; ++j) is[j] = inv_std[cols[j]];
    }
    if (mean) {      // uniform
#pragma unroll
        for (int j = 0; j < D; ++j) mn[j] = mean[cols[j]];
    }
    nbias = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        double wu = pu[j], wd = pd[j];
        if (ARS) {   // ars_agent.py:141-142
            wu = __dadd_rn(wu, sgn * __dmul_rn(nu, du[j]));
            wd = __dadd_rn(wd, sgn * __dmul_rn(nu, dd[j]));
        }
        if (inv_std) {   // environment.py:32-33
            wu = __dmul_rn(wu, is[j]);
            wd = __dmul_rn(wd, is[j]);
        }
        const double up = (seg >= 1) ? wu : 0.0;
        const double dn = (seg <= M - 1) ? wd : 0.0;
        V[j] = c12 * (up - dn);
        if (mean) nbias = __builtin_fma(-V[j], mn[j], nbias);
    }
}

}  // namespace

// ------------------------------------------------------------------------------------
// What crosses the files: the plan of a rollout launch, and one table of launch functions per kernel form.  (The
// attribute holds for one block of the namespace: the files that define the tables repeat it.)
namespace sw_launch __attribute__((visibility("hidden"))) {

// The four forms of a rollout launch (above), chosen in one place: plan_rollouts(), swimmer_abi.hip.
enum class Form { Oct3, Quad3, Row, Lane };
constexpr Form kForms[] = {Form::Oct3, Form::Quad3, Form::Row, Form::Lane};

constexpr int form_block(Form f)
{
    return f == Form::Oct3 ? kOctBlock : f == Form::Row ? kRowBlock : kRollBlock;
}

// Workgroup size of the covariance pass that a launch of form f leaves owed: the pass rides along in a
// launch of the same form, or is flushed with that form's workgroups.  The lane kernel carries no side
// job, so its pass is always the flushed one, with the standalone pass's kMomBlock.
constexpr int owed_cov_block(Form f) { return f == Form::Lane ? kMomBlock : form_block(f); }

struct RolloutPlan {
    Form form;
    int block;                 // threads per workgroup
    unsigned rollout_blocks;   // workgroups that run rollouts (a side job's come behind them)
    bool carries_side;         // the form's kernels take a SideJob
};

// What the rollout kernels take besides the model and the batch.  Plain rollouts (sw_rollout_f64): one
// policy per rollout, no deltas.  ARS rollouts: one policy, +-nu deltas[dir_begin + i], no state0 /
// final_state.
struct RolloutArgs {
    const double *policies, *deltas;
    int64_t dir_begin;
    double nu;
    const double *mean, *inv_std, *state0;
    double *returns, *traj, *final_state, *moments;
    int32_t *status;
};

// What a rollout launch of the ARS pipeline is asked to carry besides its rollouts: the progress flag and the
// covariance pass over the previous iteration's trajectories (cov_traj == nullptr: none).  The launch function
// makes the kernels' SideJob (swimmer_cov.h) of it.
struct SideWork {
    uint32_t *flag;
    uint32_t flag_value;
    const double *cov_traj;
    double *cov_acc;
    int64_t cov_rolls;
    int32_t cov_H;
};

// Tiling of a covariance pass over traj [H][D][n_roll] for workgroups of `block` threads:
// nbx tiles of `block` rollouts x ny tiles of tchunk steps.  A function of (n_roll, H, block)
// only, so a pass always sums in the same order (bit-reproducible results).
struct CovTiling {
    uint32_t nbx, ny;
    int32_t tchunk;
};

// riding: the pass rides along in a rollout launch (or is the flush of a pass owed to one: same tiling,
// same order of summation).  Otherwise it is the standalone pass of sw_traj_moments_f64, alone on the chip.
CovTiling cov_tiling(int64_t n_roll, int32_t H, int block, int D, bool riding);   // swimmer_cov.hip
int launch_traj_moments(const sw_params *p, int64_t n_roll, int32_t H, const double *traj, double *acc, int block,
                        bool riding, void *stream);

// The types of a form's launch functions, one per operation.  The functions are private to the file of the form's
// kernels; they return launch_status(), or SW_ERR_SEGMENTS for an n the form has no kernel for.  The entry points have
// validated the parameters and the sizes, and cleared stale errors, already.
// Rollouts (launch_rollouts, swimmer_abi.hip); side: pipeline only, and not for the lane form
// (RolloutPlan::carries_side).
using RolloutLauncher = int(const sw_params *p, const RolloutPlan &plan, bool ars, int64_t n_roll, int32_t H,
                            const RolloutArgs &a, hipStream_t stream, const SideWork *side);
// The ARS simulator gate (sw_ars_gate_f64): a = the ARS rollouts' arguments without trajectories / moments.
using GateLauncher = int(const sw_params *sim, const RolloutPlan &plan, int64_t n_roll, int32_t H,
                         const RolloutArgs &a, double gate_thr, int32_t *admit, hipStream_t stream);
// The ARS rollouts of n_agent agents in one launch (sw_ars_rollouts_multi_f64).  Every array is the single-agent
// array of sw_ars_rollouts_f64 once per agent, agent-major and dense: policy [n_agent][m][d], deltas
// [n_agent][n_dir][m][d], mean / inv_std [n_agent][d] (both null: V1), returns / status [n_agent][2 n_dir],
// moments [n_agent][ceil(2 n_dir / 16)][2d] (null: none).
struct MultiArgs {
    const double *policy, *deltas, *mean, *inv_std;
    double *returns, *moments;
    int32_t *status;
};
// Slots (rollouts a workgroup has lanes for) per workgroup of a form: the granule an agent's rollouts are padded to,
// so that no workgroup -- and no 16-rollout moment row -- ever holds two agents.
constexpr int form_slots(Form f) { return f == Form::Lane ? kRollBlock : kMomGroup; }
// n_roll = 2 n_dir rollouts per agent; grid = (workgroups per agent, n_agent), blocks of plan.block threads.
using MultiLauncher = int(const sw_params *p, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, int32_t H,
                          const MultiArgs &a, double nu, hipStream_t stream);
inline dim3 multi_grid(const RolloutPlan &plan, int64_t n_agent, int64_t n_roll)
{
    const int per = form_slots(plan.form);
    return dim3((unsigned)((n_roll + per - 1) / per), (unsigned)n_agent);
}
// one launch of a multi-agent kernel on that grid
template <class Kernel, class... Args>
void launch_agent_grid(Kernel *kernel, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, hipStream_t stream,
                       const Args &...args)
{
    hipLaunchKernelGGL(kernel, multi_grid(plan, n_agent, n_roll), dim3(plan.block), 0, stream, args...);
}
// The safe half of a batch of agents (sw_ars_gate_multi_f64, sw_ars_rollouts_multi_counted_f64): MultiArgs plus, for
// the gate, every agent's simulator (sim [n_agent][3] = l_i, m_i, k), simulator threshold and admit flags
// [n_agent][n_dir]; for the counted rollouts every agent's direction count [n_agent] (n_roll is then the maximum and
// sets the strides).  A struct of its own: MultiArgs is a kernel argument of the ars_multi_* kernels as it is.
struct SafeMultiArgs {
    const double *policy, *deltas, *mean, *inv_std;
    double *returns, *moments;
    int32_t *status;
    const double *sim, *sim_thresh;
    int32_t *admit;
    const int32_t *count;
};
using SafeMultiLauncher = int(const sw_params *p, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, int32_t H,
                              const SafeMultiArgs &a, double nu, hipStream_t stream);
// The member launch of the ensemble gate (sw_ars_gate_ensemble_f64): every agent's gate in n_sim simulators, grid
// (workgroups of one agent, n_agent * n_sim).  policy / deltas / mean / inv_std / sim_thresh are per AGENT as in
// SafeMultiArgs; sim [n_agent][n_sim][3] and the outputs -- returns / status [n_agent][n_sim][2 n_dir], admit
// [n_agent][n_sim][n_dir] -- are per MEMBER.  A struct of its own: SafeMultiArgs is a kernel argument of the
// ars_gate_multi_* and ars_counted_* kernels as it is.
struct EnsembleArgs {
    const double *policy, *deltas, *mean, *inv_std;
    double *returns;
    int32_t *status;
    const double *sim, *sim_thresh;
    int32_t *admit;
    int32_t n_sim;
};
// n_member = n_agent * n_sim: the grid's second dimension
using EnsembleLauncher = int(const sw_params *p, const RolloutPlan &plan, int64_t n_member, int64_t n_roll, int32_t H,
                             const EnsembleArgs &a, double nu, hipStream_t stream);
// Safe exploration (sw_safe_rollouts_f64).
using SafeLauncher = int(const sw_params *real, const sw_params *sim, const RolloutPlan &plan, int64_t n_roll,
                         int32_t H, const double *policies, int32_t cost_kind, int32_t cost_index, double sim_thresh,
                         double real_thresh, double *returns, double *traj, int32_t *first_refused,
                         int32_t *violations, int32_t *status, hipStream_t stream);
// Safe exploration for the ARS rollouts of n_agent agents (sw_safe_ars_rollouts_multi_f64): agent-major arrays as in
// MultiArgs, plus per agent gated [n_agent], sim [n_agent][3], sim_thresh / real_thresh [n_agent]; cost_trace
// [H][n_agent][2 n_dir]; cost_max / first_refused / violations / status [n_agent][2 n_dir] (null: not wanted).
struct SafeArsMultiArgs {
    const double *policy, *deltas;
    const int32_t *gated;
    const double *sim, *sim_thresh, *real_thresh;
    double *returns, *cost_trace, *cost_max;
    int32_t *first_refused, *violations, *status;
};
using SafeArsMultiLauncher = int(const sw_params *real, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll,
                                 int32_t H, const SafeArsMultiArgs &a, double nu, int32_t cost_kind,
                                 int32_t cost_index, hipStream_t stream);
// A form's launch functions by operation, defined in the file of the form's kernels; nullptr: the form has no kernel
// for it, and plan_rollouts() hands the launch to the lane form, which has them all.  (Const members, not const tables:
// the device pass of the compile would emit a const table too, and has no launch functions to point it at.)
struct FormLaunchers {
    RolloutLauncher *const rollouts;
    GateLauncher *const gate;
    MultiLauncher *const multi;
    SafeMultiLauncher *const gate_multi, *const counted;
    SafeLauncher *const safe;                     // (none in the quad form)
    SafeArsMultiLauncher *const safe_ars_multi;   // (mirror-quad and lane only; swimmer_rollout_safe_multi.hip)
    EnsembleLauncher *const gate_ensemble;        // the member launch of sw_ars_gate_ensemble_f64
};
extern FormLaunchers kOct3Launchers, kQuad3Launchers, kRowLaunchers, kLaneLaunchers;

}  // namespace sw_launch
