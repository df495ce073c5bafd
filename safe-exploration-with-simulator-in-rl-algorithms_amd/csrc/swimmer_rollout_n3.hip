// swimmer_rollout_n3.hip -- n = 3 rollouts with one segment per lane: the quad kernel (swimmer_quad3.h) and the
// mirror-quad kernel with lane roles (swimmer_oct3.h) and its two packed-record forms, their ARS gate kernels and the
// mirror-quad safe-exploration kernel.  (One file: the three forms share load_policy_row<8, 2, ...> and the riding covariance tile.)
#include "swimmer_cov.h"
#include "swimmer_quad3.h"
#include "swimmer_oct3.h"

namespace {

// ------------------------------------------------------------------------------------
// n = 3, one segment per lane (swimmer_quad3.h): 16 rollouts per 64-thread workgroup.
// TRAJ / MOM are compile-time so the hot loop carries no per-step uniform branches.
template <bool ARS, bool TRAJ, bool MOM>
__global__ void __launch_bounds__(kRollBlock)
rollout_quad3_kernel(sw::Consts C, int64_t n_roll, int32_t H, const double *__restrict__ policies,
                     const double *__restrict__ deltas, int64_t dir_begin, double nu,
                     const double *__restrict__ mean, const double *__restrict__ inv_std,
                     const double *__restrict__ state0, double *__restrict__ returns,
                     double *__restrict__ traj, double *__restrict__ final_state,
                     double *__restrict__ moments, int32_t *__restrict__ status, SideJob side)
{
#define SW_GATE_BODY 0
#include "swimmer_rollout_quad3.inc"
#undef SW_GATE_BODY
}

// The ARS simulator gate (sw_ars_gate_f64) in the quad form (body: swimmer_rollout_quad3.inc).
__global__ void __launch_bounds__(kRollBlock)
ars_gate_quad3_kernel(sw::Consts C, int64_t n_roll, int32_t H, const double *__restrict__ policies,
                      const double *__restrict__ deltas, int64_t dir_begin, double nu,
                      const double *__restrict__ mean, const double *__restrict__ inv_std, double gate_thr,
                      int32_t *__restrict__ admit, double *__restrict__ returns, int32_t *__restrict__ status,
                      SideJob side)
{
    constexpr bool ARS = true, TRAJ = false, MOM = false;
    const double *const state0 = nullptr;
    double *const traj = nullptr;
    double *const final_state = nullptr;
    double *const moments = nullptr;
#define SW_GATE_BODY 1
#include "swimmer_rollout_quad3.inc"
#undef SW_GATE_BODY
}

// ------------------------------------------------------------------------------------
// n = 3 with lane roles (swimmer_oct3.h): two mirror quads per rollout, 8 rollouts per wave, two
// waves = 16 rollouts = one V2 moment row per 128-thread workgroup.
template <bool ARS, bool TRAJ, bool MOM>
__global__ void __launch_bounds__(kOctBlock)
rollout_oct3_kernel(sw::Consts C, int64_t n_roll, int32_t H, const double *__restrict__ policies,
                    const double *__restrict__ deltas, int64_t dir_begin, double nu,
                    const double *__restrict__ mean, const double *__restrict__ inv_std,
                    const double *__restrict__ state0, double *__restrict__ returns,
                    double *__restrict__ traj, double *__restrict__ final_state,
                    double *__restrict__ moments, int32_t *__restrict__ status, SideJob side)
{
#define SW_GATE_BODY 0
#include "swimmer_rollout_oct3.inc"
#undef SW_GATE_BODY
}

// The ARS simulator gate (sw_ars_gate_f64) in the mirror-quad form (body: swimmer_rollout_oct3.inc).
__global__ void __launch_bounds__(kOctBlock)
ars_gate_oct3_kernel(sw::Consts C, int64_t n_roll, int32_t H, const double *__restrict__ policies,
                     const double *__restrict__ deltas, int64_t dir_begin, double nu,
                     const double *__restrict__ mean, const double *__restrict__ inv_std, double gate_thr,
                     int32_t *__restrict__ admit, double *__restrict__ returns, int32_t *__restrict__ status,
                     SideJob side)
{
    constexpr bool ARS = true, TRAJ = false, MOM = false;
    const double *const state0 = nullptr;
    double *const traj = nullptr;
    double *const final_state = nullptr;
    double *const moments = nullptr;
#define SW_GATE_BODY 1
#include "swimmer_rollout_oct3.inc"
#undef SW_GATE_BODY
}

// The mirror-quad rollout with capture and V2 moments in the PACKED record form (body: swimmer_rollout_octp3.inc): the
// eight state components of a rollout on its eight lanes, ONE trajectory store and ONE moment pair per step where
// rollout_oct3_kernel<ARS, true, true> has three stores and six accumulates; same outputs, bit for bit.
template <bool ARS>
__global__ void __launch_bounds__(kOctBlock)
rollout_octp3_kernel(sw::Consts C, int64_t n_roll, int32_t H, const double *__restrict__ policies,
                     const double *__restrict__ deltas, int64_t dir_begin, double nu,
                     const double *__restrict__ mean, const double *__restrict__ inv_std,
                     const double *__restrict__ state0, double *__restrict__ returns,
                     double *__restrict__ traj, double *__restrict__ final_state,
                     double *__restrict__ moments, int32_t *__restrict__ status, SideJob side)
{
#define SW_OCTP_LEAN 0
#define SW_OCTP_NEXT_E 0
#include "swimmer_rollout_octp3.inc"
#undef SW_OCTP_NEXT_E
#undef SW_OCTP_LEAN
}

// The packed record form with a leaner step (the same body with SW_OCTP_LEAN 1; its header lists the three places that
// differ): the trajectory stores take their scalar offsets from seven loop-invariant SGPRs and the trip's base from
// the vector offset, bumped once per trip, and the range test branches on vcc.  21 scalar instructions fewer per trip
// of eight steps; every output has rollout_octp3_kernel's bits.  SW_FLAG_CAPTURE_LEAN_V1 launches it (the default of
// a launch with capture and V2 moments is rollout_octs3_kernel, below); SW_FLAG_CAPTURE_PACKED_V1 keeps
// rollout_octp3_kernel.
template <bool ARS>
__global__ void __launch_bounds__(kOctBlock)
rollout_octl3_kernel(sw::Consts C, int64_t n_roll, int32_t H, const double *__restrict__ policies,
                     const double *__restrict__ deltas, int64_t dir_begin, double nu,
                     const double *__restrict__ mean, const double *__restrict__ inv_std,
                     const double *__restrict__ state0, double *__restrict__ returns,
                     double *__restrict__ traj, double *__restrict__ final_state,
                     double *__restrict__ moments, int32_t *__restrict__ status, SideJob side)
{
#define SW_OCTP_LEAN 1
#define SW_OCTP_NEXT_E 0
#include "swimmer_rollout_octp3.inc"
#undef SW_OCTP_NEXT_E
#undef SW_OCTP_LEAN
}

// The lean kernel with the neighbour's matrix entry (the same body with SW_OCTP_NEXT_E 1): Q(i+1, i+2) of a lane's
// rotated 3x3 system is lane i+1's Q(i, i+1), bit for bit, so a step takes it through two DPP moves and forms neither
// cos(th_i1 - th_i2) nor its product with t12 (swimmer_oct3.h: oct3_geometry_next_e / oct3_dynamics_next_e), and its
// main loop runs sixteen steps per trip (SW_OCTS_TRIP16).  Every output has rollout_octl3_kernel's bits.  The default of a launch with capture and V2 moments;
// SW_FLAG_CAPTURE_LEAN_V1 keeps rollout_octl3_kernel.
template <bool ARS>
__global__ void __launch_bounds__(kOctBlock)
rollout_octs3_kernel(sw::Consts C, int64_t n_roll, int32_t H, const double *__restrict__ policies,
                     const double *__restrict__ deltas, int64_t dir_begin, double nu,
                     const double *__restrict__ mean, const double *__restrict__ inv_std,
                     const double *__restrict__ state0, double *__restrict__ returns,
                     double *__restrict__ traj, double *__restrict__ final_state,
                     double *__restrict__ moments, int32_t *__restrict__ status, SideJob side)
{
#define SW_OCTP_LEAN 1
#define SW_OCTP_NEXT_E 1
#include "swimmer_rollout_octp3.inc"
#undef SW_OCTP_NEXT_E
#undef SW_OCTP_LEAN
}

// ------------------------------------------------------------------------------------
// sw_ars_rollouts_multi_f64 in the quad and the mirror-quad form: the ARS rollouts of many agents in one launch, the
// form's body behind the per-agent view (swimmer_rollout_multi.inc).  No capture, no side job (kNoSide).
#define SW_MULTI_N 3
template <bool MOM>
__global__ void __launch_bounds__(kRollBlock)
ars_multi_quad3_kernel(sw::Consts C, int64_t n_roll, int32_t H, sw_launch::MultiArgs all, double nu, SideJob side)
{
    constexpr bool ARS = true, TRAJ = false;
#include "swimmer_rollout_multi.inc"
#define SW_GATE_BODY 0
#include "swimmer_rollout_quad3.inc"
#undef SW_GATE_BODY
}

template <bool MOM>
__global__ void __launch_bounds__(kOctBlock)
ars_multi_oct3_kernel(sw::Consts C, int64_t n_roll, int32_t H, sw_launch::MultiArgs all, double nu, SideJob side)
{
    constexpr bool ARS = true, TRAJ = false;
#include "swimmer_rollout_multi.inc"
#define SW_GATE_BODY 0
#include "swimmer_rollout_oct3.inc"
#undef SW_GATE_BODY
}

// sw_ars_gate_multi_f64 and sw_ars_rollouts_multi_counted_f64 in the two n = 3 forms: the safe half of a batch of
// agents.  The gate kernels are the form's body with SW_GATE_BODY 1 behind the view with SW_MULTI_GATE 1 (C, gate_thr
// and admit per agent); the counted kernels are ars_multi_*_kernel with the agent's rollout count read in the view.
#define SW_MULTI_SLOTS kMomGroup
#define SW_MULTI_GATE 1
#define SW_MULTI_PAD quad_gate_multi_loop_pad()
__global__ void __launch_bounds__(kRollBlock)
ars_gate_multi_quad3_kernel(sw::Consts base, int64_t n_roll, int32_t H, sw_launch::SafeMultiArgs all, double nu,
                            SideJob side)
{
    constexpr bool ARS = true, TRAJ = false, MOM = false;
#include "swimmer_rollout_multi.inc"
#define SW_GATE_BODY 1
#include "swimmer_rollout_quad3.inc"
#undef SW_GATE_BODY
}
#undef SW_MULTI_PAD

#define SW_MULTI_PAD oct_gate_multi_loop_pad()
__global__ void __launch_bounds__(kOctBlock)
ars_gate_multi_oct3_kernel(sw::Consts base, int64_t n_roll, int32_t H, sw_launch::SafeMultiArgs all, double nu,
                           SideJob side)
{
    constexpr bool ARS = true, TRAJ = false, MOM = false;
#include "swimmer_rollout_multi.inc"
#define SW_GATE_BODY 1
#include "swimmer_rollout_oct3.inc"
#undef SW_GATE_BODY
}
#undef SW_MULTI_PAD

// The member launch of sw_ars_gate_ensemble_f64 in the two n = 3 forms: the same bodies behind the view with
// SW_MULTI_ENSEMBLE 1 (blockIdx.y = agent * n_sim + member: the agent's policy and deltas, the member's simulator and
// outputs).
#define SW_MULTI_ENSEMBLE 1
#define SW_MULTI_PAD quad_gate_ens_loop_pad()
__global__ void __launch_bounds__(kRollBlock)
ars_gate_ens_quad3_kernel(sw::Consts base, int64_t n_roll, int32_t H, sw_launch::EnsembleArgs all, double nu,
                          SideJob side)
{
    constexpr bool ARS = true, TRAJ = false, MOM = false;
#include "swimmer_rollout_multi.inc"
#define SW_GATE_BODY 1
#include "swimmer_rollout_quad3.inc"
#undef SW_GATE_BODY
}
#undef SW_MULTI_PAD

#define SW_MULTI_PAD oct_gate_ens_loop_pad()
__global__ void __launch_bounds__(kOctBlock)
ars_gate_ens_oct3_kernel(sw::Consts base, int64_t n_roll, int32_t H, sw_launch::EnsembleArgs all, double nu,
                         SideJob side)
{
    constexpr bool ARS = true, TRAJ = false, MOM = false;
#include "swimmer_rollout_multi.inc"
#define SW_GATE_BODY 1
#include "swimmer_rollout_oct3.inc"
#undef SW_GATE_BODY
}
#undef SW_MULTI_PAD
#undef SW_MULTI_ENSEMBLE
#undef SW_MULTI_GATE

#define SW_MULTI_COUNTED 1
#define SW_MULTI_PAD quad_counted_loop_pad(MOM)
template <bool MOM>
__global__ void __launch_bounds__(kRollBlock)
ars_counted_quad3_kernel(sw::Consts C, int64_t n_roll_max, int32_t H, sw_launch::SafeMultiArgs all, double nu,
                         SideJob side)
{
    constexpr bool ARS = true, TRAJ = false;
#include "swimmer_rollout_multi.inc"
#define SW_GATE_BODY 0
#include "swimmer_rollout_quad3.inc"
#undef SW_GATE_BODY
}
#undef SW_MULTI_PAD

#define SW_MULTI_PAD oct_counted_loop_pad(MOM)
template <bool MOM>
__global__ void __launch_bounds__(kOctBlock)
ars_counted_oct3_kernel(sw::Consts C, int64_t n_roll_max, int32_t H, sw_launch::SafeMultiArgs all, double nu,
                        SideJob side)
{
    constexpr bool ARS = true, TRAJ = false;
#include "swimmer_rollout_multi.inc"
#define SW_GATE_BODY 0
#include "swimmer_rollout_oct3.inc"
#undef SW_GATE_BODY
}
#undef SW_MULTI_PAD
#undef SW_MULTI_COUNTED
#undef SW_MULTI_SLOTS
#undef SW_MULTI_N

// ------------------------------------------------------------------------------------
// The safe-exploration gate (safe_rollout_kernel above has the semantics) for n = 3 in the MIRROR-QUAD form of
// rollout_oct3_kernel: two quads of eight lanes per rollout, lane roles, reduced angles.  The geometry of a step
// (sin / cos, cos(th_i - th_k), ...) depends on the angles only and is therefore SHARED by the simulator's look-ahead
// and the real step: per step one geometry, two `oct3_dynamics` (simulator constants on copies of Gdot / thetadot,
// real constants), the cost of the simulated next state on the lanes that own the observed quantity, one AND over
// the rollout's eight lanes (three DPP-ANDs: the two mirror quads differ by rounding, the decision must not), and
// the real step committed through selects.  170 instructions per env-step (186 with the violation count) instead of
// ~640 in the lane form: 0.354 ms per 1024 gated rollouts x 1000 steps against 1.13 ms (profiles/r04_z).
// A refused rollout keeps recomputing the same refused step (its state no longer changes), as in the reference.
template <bool TRAJ, bool VIOL>
__global__ void __launch_bounds__(kOctBlock)
safe_rollout_oct3_kernel(sw::Consts Cr, sw::Consts Cs, double tq_ratio, int64_t n_roll, int32_t H,
                         const double *__restrict__ policies, int32_t cost_kind, int32_t cost_index,
                         double sim_thresh, double real_thresh, double *__restrict__ returns,
                         double *__restrict__ traj, int32_t *__restrict__ first_refused,
                         int32_t *__restrict__ violations, int32_t *__restrict__ status)
{
#define SW_SAFE_MULTI 0
#include "swimmer_rollout_safe_oct3.inc"
#undef SW_SAFE_MULTI
}

// ---- host: the form's launch functions (private) and its table of them (sw_launch) ----
using namespace sw_launch;

int launch_oct3(const sw_params *p, const RolloutPlan &plan, bool ars, int64_t n_roll, int32_t H, const RolloutArgs &a,
                hipStream_t stream, const SideWork *side)
{
    // capture + V2 moments: the packed record form with the lean step and the neighbour's matrix entry, unless
    // SW_FLAG_CAPTURE_LEAN_V1 asks for the lean kernel before it, SW_FLAG_CAPTURE_PACKED_V1 for the first packed
    // kernel or SW_FLAG_CAPTURE_SPLIT for the three-store kernel (validate_params: at most one of the three)
    if (a.traj && a.moments && !(p->flags & SW_FLAG_CAPTURE_SPLIT)) {
        with_bools([&](auto ARS, auto V1, auto LEAN_V1) {
            if constexpr (V1.value)
                launch_segment_per_lane(rollout_octp3_kernel<ARS.value>, p, plan, n_roll, H, a, stream, side);
            else if constexpr (LEAN_V1.value)
                launch_segment_per_lane(rollout_octl3_kernel<ARS.value>, p, plan, n_roll, H, a, stream, side);
            else
                launch_segment_per_lane(rollout_octs3_kernel<ARS.value>, p, plan, n_roll, H, a, stream, side);
        }, ars, (p->flags & SW_FLAG_CAPTURE_PACKED_V1) != 0, (p->flags & SW_FLAG_CAPTURE_LEAN_V1) != 0);
        return launch_status();
    }
    with_bools([&](auto ARS, auto TRAJ, auto MOM) {
        launch_segment_per_lane(rollout_oct3_kernel<ARS.value, TRAJ.value, MOM.value>, p, plan, n_roll, H, a, stream,
                                side);
    }, ars, a.traj != nullptr, a.moments != nullptr);
    return launch_status();
}

int launch_quad3(const sw_params *p, const RolloutPlan &plan, bool ars, int64_t n_roll, int32_t H,
                 const RolloutArgs &a, hipStream_t stream, const SideWork *side)
{
    with_bools([&](auto ARS, auto TRAJ, auto MOM) {
        launch_segment_per_lane(rollout_quad3_kernel<ARS.value, TRAJ.value, MOM.value>, p, plan, n_roll, H, a, stream,
                                side);
    }, ars, a.traj != nullptr, a.moments != nullptr);
    return launch_status();
}

int launch_gate_oct3(const sw_params *sim, const RolloutPlan &plan, int64_t n_roll, int32_t H, const RolloutArgs &a,
                     double gate_thr, int32_t *admit, hipStream_t stream)
{
    launch_gate_segment_per_lane(ars_gate_oct3_kernel, sim, plan, n_roll, H, a, gate_thr, admit, stream);
    return launch_status();
}

int launch_gate_quad3(const sw_params *sim, const RolloutPlan &plan, int64_t n_roll, int32_t H, const RolloutArgs &a,
                      double gate_thr, int32_t *admit, hipStream_t stream)
{
    launch_gate_segment_per_lane(ars_gate_quad3_kernel, sim, plan, n_roll, H, a, gate_thr, admit, stream);
    return launch_status();
}

int launch_multi_oct3(const sw_params *p, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, int32_t H,
                      const MultiArgs &a, double nu, hipStream_t stream)
{
    with_bools([&](auto MOM) {
        launch_agent_grid(ars_multi_oct3_kernel<MOM.value>, plan, n_agent, n_roll, stream, make_consts(p), n_roll, H,
                          a, nu, kNoSide);
    }, a.moments != nullptr);
    return launch_status();
}

int launch_multi_quad3(const sw_params *p, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, int32_t H,
                       const MultiArgs &a, double nu, hipStream_t stream)
{
    with_bools([&](auto MOM) {
        launch_agent_grid(ars_multi_quad3_kernel<MOM.value>, plan, n_agent, n_roll, stream, make_consts(p), n_roll, H,
                          a, nu, kNoSide);
    }, a.moments != nullptr);
    return launch_status();
}

int launch_gate_multi_oct3(const sw_params *p, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, int32_t H,
                           const SafeMultiArgs &a, double nu, hipStream_t stream)
{
    launch_agent_grid(ars_gate_multi_oct3_kernel, plan, n_agent, n_roll, stream, make_consts(p), n_roll, H, a, nu,
                      kNoSide);
    return launch_status();
}

int launch_gate_multi_quad3(const sw_params *p, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, int32_t H,
                            const SafeMultiArgs &a, double nu, hipStream_t stream)
{
    launch_agent_grid(ars_gate_multi_quad3_kernel, plan, n_agent, n_roll, stream, make_consts(p), n_roll, H, a, nu,
                      kNoSide);
    return launch_status();
}

int launch_gate_ens_oct3(const sw_params *p, const RolloutPlan &plan, int64_t n_member, int64_t n_roll, int32_t H,
                         const EnsembleArgs &a, double nu, hipStream_t stream)
{
    launch_agent_grid(ars_gate_ens_oct3_kernel, plan, n_member, n_roll, stream, make_consts(p), n_roll, H, a, nu,
                      kNoSide);
    return launch_status();
}

int launch_gate_ens_quad3(const sw_params *p, const RolloutPlan &plan, int64_t n_member, int64_t n_roll, int32_t H,
                          const EnsembleArgs &a, double nu, hipStream_t stream)
{
    launch_agent_grid(ars_gate_ens_quad3_kernel, plan, n_member, n_roll, stream, make_consts(p), n_roll, H, a, nu,
                      kNoSide);
    return launch_status();
}

int launch_counted_oct3(const sw_params *p, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, int32_t H,
                        const SafeMultiArgs &a, double nu, hipStream_t stream)
{
    with_bools([&](auto MOM) {
        launch_agent_grid(ars_counted_oct3_kernel<MOM.value>, plan, n_agent, n_roll, stream, make_consts(p), n_roll,
                          H, a, nu, kNoSide);
    }, a.moments != nullptr);
    return launch_status();
}

int launch_counted_quad3(const sw_params *p, const RolloutPlan &plan, int64_t n_agent, int64_t n_roll, int32_t H,
                         const SafeMultiArgs &a, double nu, hipStream_t stream)
{
    with_bools([&](auto MOM) {
        launch_agent_grid(ars_counted_quad3_kernel<MOM.value>, plan, n_agent, n_roll, stream, make_consts(p), n_roll,
                          H, a, nu, kNoSide);
    }, a.moments != nullptr);
    return launch_status();
}

// n = 3, up to 8192 rollouts: the mirror-quad form (one geometry, two dynamics per env-step)
int launch_safe_oct3(const sw_params *real, const sw_params *sim, const RolloutPlan &plan, int64_t n_roll, int32_t H,
                     const double *policies, int32_t cost_kind, int32_t cost_index, double sim_thresh,
                     double real_thresh, double *returns, double *traj, int32_t *first_refused, int32_t *violations,
                     int32_t *status, hipStream_t stream)
{
    const sw::Consts Cr = make_consts(real), Cs = make_consts(sim);
    const double tq_ratio = Cs.c12 / Cr.c12;
    with_bools([&](auto TRAJ, auto VIOL) {
        hipLaunchKernelGGL((safe_rollout_oct3_kernel<TRAJ.value, VIOL.value>), dim3(plan.rollout_blocks),
                           dim3(plan.block), 0, stream, Cr, Cs, tq_ratio, n_roll, H, policies, cost_kind, cost_index,
                           sim_thresh, real_thresh, returns, traj, first_refused, violations, status);
    }, traj != nullptr, violations != nullptr);
    return launch_status();
}
SafeArsMultiLauncher launch_safe_ars_multi_oct3;   // swimmer_rollout_safe_multi.hip, later in the translation unit

}  // namespace

namespace sw_launch __attribute__((visibility("hidden"))) {
FormLaunchers kOct3Launchers = {launch_oct3,         launch_gate_oct3, launch_multi_oct3, launch_gate_multi_oct3,
                                launch_counted_oct3, launch_safe_oct3, launch_safe_ars_multi_oct3,
                                launch_gate_ens_oct3};
FormLaunchers kQuad3Launchers = {launch_quad3,         launch_gate_quad3, launch_multi_quad3, launch_gate_multi_quad3,
                                 launch_counted_quad3, /*safe=*/nullptr,  /*safe_ars_multi=*/nullptr,
                                 launch_gate_ens_quad3};
}  // namespace sw_launch
