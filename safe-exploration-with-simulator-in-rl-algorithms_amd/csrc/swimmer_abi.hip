// swimmer_abi.hip -- the rollout side of the C ABI of include/swimmer_hip.h: which kernel form a launch takes
// (plan_rollouts, plan_multi) and the one dispatch over the forms' tables of launch functions (launchers), the rollout /
// gate / safe-rollout entry points, the issue probe, and the native ARS iteration pipeline.  (The step, update and
// covariance entry points are in the files of their kernels.)
#include <chrono>
#include <new>
#include <vector>

#include "swimmer_launch.h"

using namespace sw_launch;

namespace {

// ------------------------------------------------------------------------------------
// Calibration of the latency-bound rollouts' ceiling on THIS device: one wave issuing `trips` x 64
// independent instructions of one class (mode 0: v_fma_f64 on 8 accumulators; mode 1: v_mov_b32).
// bench.py times it with HIP events and prices the rollout kernel's per-step instruction mix
// with the two intervals (roofline.issue_bound).
// A grid of such waves (sw_issue_probe_grid: 256 workgroups x 4 waves = one wave on every SIMD) gives the
// same intervals with the WHOLE chip issuing -- f64 on every SIMD lowers the clock the chip sustains.
__global__ void __launch_bounds__(256) issue_probe_kernel(int32_t trips, int32_t mode, double *out)
{
    double a0 = 1.0 + threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5,
           a6 = a0 + 6, a7 = a0 + 7;
    const double m = 1.0000001, c = 1e-9;
    int b0 = threadIdx.x, b1 = b0 + 1, b2 = b0 + 2, b3 = b0 + 3, b4 = b0 + 4, b5 = b0 + 5, b6 = b0 + 6,
        b7 = b0 + 7;
#define SW_FMA8 "v_fma_f64 %0, %0, %8, %9\n v_fma_f64 %1, %1, %8, %9\n v_fma_f64 %2, %2, %8, %9\n" \
                "v_fma_f64 %3, %3, %8, %9\n v_fma_f64 %4, %4, %8, %9\n v_fma_f64 %5, %5, %8, %9\n" \
                "v_fma_f64 %6, %6, %8, %9\n v_fma_f64 %7, %7, %8, %9\n"
#define SW_MOV8 "v_mov_b32 %0, %1\n v_mov_b32 %1, %2\n v_mov_b32 %2, %3\n v_mov_b32 %3, %4\n" \
                "v_mov_b32 %4, %5\n v_mov_b32 %5, %6\n v_mov_b32 %6, %7\n v_mov_b32 %7, %0\n"
    if (mode == 0) {
        for (int32_t t = 0; t < trips; ++t)
            asm volatile(SW_FMA8 SW_FMA8 SW_FMA8 SW_FMA8 SW_FMA8 SW_FMA8 SW_FMA8 SW_FMA8
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                         : "v"(m), "v"(c));
    } else {
        for (int32_t t = 0; t < trips; ++t)
            asm volatile(SW_MOV8 SW_MOV8 SW_MOV8 SW_MOV8 SW_MOV8 SW_MOV8 SW_MOV8 SW_MOV8
                         : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7));
    }
#undef SW_FMA8
#undef SW_MOV8
    // (every wave of a grid writes the same 64 doubles' worth of don't-care values)
    out[threadIdx.x % kWave] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + (double)(b0 ^ b1 ^ b2 ^ b3 ^ b4 ^ b5 ^ b6 ^ b7);
}

// The one dispatch over the forms: every launch goes through the table of its plan's form.
const FormLaunchers &launchers(Form form)
{
    switch (form) {
    case Form::Oct3: return kOct3Launchers;
    case Form::Quad3: return kQuad3Launchers;
    case Form::Row: return kRowLaunchers;
    case Form::Lane: break;
    }
    return kLaneLaunchers;
}

// Kernel choice for rollouts: a segment-per-lane kernel while it still finds idle SIMDs, the
// lane-per-rollout kernel beyond; sw_params.flags can force either.
//  * n = 3 with lane roles (two mirror quads per rollout, swimmer_oct3.h): 8 rollouts per wave, so it
//    keeps one wave per SIMD up to 8192 rollouts; beyond that the quad kernel (16 per wave) takes over.
//    SWIMMER_N3_KERNEL=quad|oct overrides the default (measurement knob).
//  * n = 4..8: the row kernel.
// op: the member of FormLaunchers that will launch the plan.  THE FALLBACK RULE: a form whose table has no entry for
// the operation hands the launch to the lane form -- safe rollouts where the quad form would run (n = 3 beyond 8192
// rollouts), the safe-ARS rollouts of a batch of agents wherever the mirror-quad form would not.
template <class Member>
RolloutPlan plan_rollouts(const sw_params *p, Member FormLaunchers::*op, int64_t n_roll, int32_t H, bool with_traj)
{
    static const char *env = getenv("SWIMMER_N3_KERNEL");
    const bool want_oct = env ? (env[0] == 'o') : SW_N3_DEFAULT_OCT;
    const bool uncapped = (p->flags & SW_FLAG_ROLLOUT_QUAD) != 0;
    Form form = Form::Lane;
    // segment-per-lane kernels: Gym model only
    if (!is_twin(p) && !(p->flags & SW_FLAG_ROLLOUT_LANE)) {
        if (p->n == 3) {
            // the quad and mirror-quad kernels address the trajectory buffer with 32-bit byte offsets
            const bool fits = !(with_traj && (int64_t)H * 8 * n_roll * 8 >= ((int64_t)1 << 32)) &&
                              n_roll < ((int64_t)1 << 25) && (uncapped || n_roll <= kQuadMaxRollouts);
            if (fits) form = want_oct && n_roll <= kOctMaxRollouts ? Form::Oct3 : Form::Quad3;
        } else if (p->n >= 4) {
            const bool fits =
                !(with_traj && (int64_t)H * (2 * p->n + 2) * n_roll * 8 >= ((int64_t)1 << 32) - 256) &&
                n_roll < ((int64_t)1 << 24) && (uncapped || n_roll <= kRowMaxRollouts);
            if (fits) form = Form::Row;
        }
    }
    if (!(launchers(form).*op)) form = Form::Lane;
    const int per_block = form_slots(form);   // rollouts per workgroup
    return RolloutPlan{form, form_block(form), (unsigned)((n_roll + per_block - 1) / per_block), form != Form::Lane};
}

// The one rollout launcher: `plan` says which form, the form's launch function which kernel and which grid.
// side: what the launch carries besides the rollouts (pipeline only; the lane form cannot take it,
// RolloutPlan::carries_side).  The public entry points have validated p and the sizes, and cleared stale errors,
// already.
int launch_rollouts(const sw_params *p, const RolloutPlan &plan, bool ars, int64_t n_roll, int32_t H,
                    const RolloutArgs &a, hipStream_t stream, const SideWork *side = nullptr)
{
    if (!a.policies || !a.returns) return SW_ERR_NULL;
    if ((a.mean == nullptr) != (a.inv_std == nullptr)) return SW_ERR_NULL;
    return launchers(plan.form).rollouts(p, plan, ars, n_roll, H, a, stream, side);
}

// The plan of a launch for n_agent agents (same model, same n_dir, same H), and THE SIZE RULE of such launches.  Every
// agent gets whole workgroups: form_slots(form) * ceil(2 n_dir / form_slots(form)) rollout slots, so a workgroup's base
// pointers are uniform and a moment row never holds two agents.  The form is chosen from the slot count of the WHOLE
// launch at the 16-slot granule: that count is what decides whether a segment-per-lane kernel still finds an idle SIMD
// per wave.  with_capture: the safe-ARS cost trace (32-bit byte offsets in the mirror-quad form, as for a trajectory).
struct MultiPlan {
    RolloutPlan plan;
    bool in_range;   // n_agent 1..65535 (grid.y), n_dir 1..2^23 (rollouts indexed like a single launch's), H >= 0
    bool fits;       // ... and fewer than 2^32 threads in the launch: the plan can be launched
};
template <class Member>
MultiPlan plan_multi(const sw_params *p, Member FormLaunchers::*op, int64_t n_agent, int64_t n_dir, int32_t H,
                     bool with_capture = false)
{
    MultiPlan m{};
    m.in_range = n_agent >= 1 && n_agent <= 65535 && n_dir >= 1 && n_dir <= ((int64_t)1 << 23) && H >= 0;
    if (!m.in_range) return m;
    const int64_t n_roll = 2 * n_dir;
    const int64_t slots = n_agent * (((n_roll + kMomGroup - 1) / kMomGroup) * kMomGroup);
    m.plan = plan_rollouts(p, op, slots, H, with_capture);
    const dim3 grid = multi_grid(m.plan, n_agent, n_roll);
    m.fits = (int64_t)grid.x * grid.y * m.plan.block < ((int64_t)1 << 32);
    return m;
}

// The fold behind the member launch of sw_ars_gate_ensemble_f64: one thread per (agent, direction) walks the agent's
// n_sim members in ascending order -- admit = AND of the members' flags, worst = their smallest return by
// `w = (x < w) ? x : w` from +inf (a NaN never replaces w), status = OR of theirs.  Plain loads and stores, no atomics
// and no hand-over between workgroups: the result does not depend on timing.  A kernel of its own, not a tail of the
// member kernels, for the reason ars_pack_admitted_kernel is one: the last workgroup to finish would have to be found
// with a device-scope counter, and the member kernels would no longer be the gate kernels' bodies.
constexpr int kFoldBlock = 256;
__global__ void __launch_bounds__(kFoldBlock)
ars_gate_fold_kernel(int64_t n_pair, int64_t n_dir, int32_t n_sim, const double *__restrict__ member_returns,
                     const int32_t *__restrict__ member_status, const int32_t *__restrict__ member_admit,
                     int32_t *__restrict__ admit, double *__restrict__ worst, int32_t *__restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * kFoldBlock + threadIdx.x;   // agent * n_dir + direction
    if (i >= n_pair) return;
    const int64_t agent = i / n_dir, dir = i - agent * n_dir;
    double w0 = __builtin_inf(), w1 = __builtin_inf();
    int32_t s0 = 0, s1 = 0, all_admit = 1;
    for (int32_t e = 0; e < n_sim; ++e) {
        const int64_t member = agent * n_sim + e;
        const double x0 = member_returns[(member * n_dir + dir) * 2], x1 = member_returns[(member * n_dir + dir) * 2 + 1];
        w0 = (x0 < w0) ? x0 : w0;
        w1 = (x1 < w1) ? x1 : w1;
        s0 |= member_status[(member * n_dir + dir) * 2];
        s1 |= member_status[(member * n_dir + dir) * 2 + 1];
        all_admit &= member_admit[member * n_dir + dir] != 0 ? 1 : 0;
    }
    admit[i] = all_admit;
    worst[2 * i] = w0;
    worst[2 * i + 1] = w1;
    if (status) {
        status[2 * i] = s0;
        status[2 * i + 1] = s1;
    }
}

}  // namespace

// =====================================================================================
extern "C" {

int sw_abi_version(void) { return SW_ABI_VERSION; }
int sw_max_segments(void) { return SW_MAX_SEGMENTS; }

const char *sw_strerror(int code)
{
    switch (code) {
    case SW_OK: return "ok";
    case SW_ERR_NULL: return "a required pointer is NULL";
    case SW_ERR_SEGMENTS: return "number of segments outside 2..8";
    case SW_ERR_SIZE: return "bad size argument";
    case SW_ERR_PARAM: return "non-finite or non-positive physical parameter";
    case SW_ERR_LAUNCH: return "HIP kernel launch failed";
    default: return "unknown error code";
    }
}

int sw_issue_probe(int32_t mode, int32_t trips, double *scratch64, void *stream)
{
    (void)hipGetLastError();
    if (!scratch64) return SW_ERR_NULL;
    if (trips < 0 || (mode != 0 && mode != 1)) return SW_ERR_SIZE;
    hipLaunchKernelGGL(issue_probe_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, trips, mode,
                       scratch64);
    return launch_status();
}

int sw_issue_probe_grid(int32_t mode, int32_t trips, int32_t workgroups, int32_t waves_per_workgroup,
                        double *scratch64, void *stream)
{
    (void)hipGetLastError();
    if (!scratch64) return SW_ERR_NULL;
    if (trips < 0 || (mode != 0 && mode != 1) || workgroups < 1 || workgroups > 65536 ||
        waves_per_workgroup < 1 || waves_per_workgroup > 4)
        return SW_ERR_SIZE;
    hipLaunchKernelGGL(issue_probe_kernel, dim3((unsigned)workgroups), dim3(kWave * waves_per_workgroup), 0,
                       (hipStream_t)stream, trips, mode, scratch64);
    return launch_status();
}

int64_t sw_moments_blocks(int64_t n_roll)
{
    return n_roll <= 0 ? 0 : (n_roll + kMomGroup - 1) / kMomGroup;
}

int sw_rollout_f64(const sw_params *p, int64_t n_roll, int32_t H, const double *policies,
                   const double *mean, const double *inv_std, const double *state0,
                   double *returns, double *traj, double *final_state, double *moments,
                   int32_t *status, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (n_roll < 0 || H < 0) return SW_ERR_SIZE;
    if (n_roll == 0) return SW_OK;
    const RolloutArgs a{policies, /*deltas=*/nullptr, /*dir_begin=*/0, /*nu=*/0.0, mean, inv_std, state0,
                        returns,  traj, final_state, moments, status};
    return launch_rollouts(p, plan_rollouts(p, &FormLaunchers::rollouts, n_roll, H, traj != nullptr), false, n_roll,
                           H, a, (hipStream_t)stream);
}

int sw_safe_rollouts_f64(const sw_params *real, const sw_params *sim, int64_t n_roll, int32_t H,
                         const double *policies, int32_t cost_kind, int32_t cost_index, double sim_thresh,
                         double real_thresh, double *returns, double *traj, int32_t *first_refused,
                         int32_t *violations, int32_t *status, void *stream)
{
    int rc = check_params(real);
    if (rc) return rc;
    rc = validate_params(sim);
    if (rc) return rc;
    if (real->n != sim->n) return SW_ERR_SEGMENTS;
    if (n_roll < 0 || H < 0) return SW_ERR_SIZE;
    if ((rc = check_cost(real, cost_kind, cost_index)) != SW_OK) return rc;
    if (!(sim_thresh == sim_thresh) || !(real_thresh == real_thresh)) return SW_ERR_PARAM;
    if (n_roll == 0) return SW_OK;
    if (!policies || !returns) return SW_ERR_NULL;
    const RolloutPlan plan = plan_rollouts(real, &FormLaunchers::safe, n_roll, H, traj != nullptr);
    return launchers(plan.form).safe(real, sim, plan, n_roll, H, policies, cost_kind, cost_index, sim_thresh,
                                     real_thresh, returns, traj, first_refused, violations, status,
                                     (hipStream_t)stream);
}

int sw_ars_rollouts_f64(const sw_params *p, int64_t dir_begin, int64_t n_dir, int32_t H,
                        const double *policy, const double *deltas, double nu, const double *mean,
                        const double *inv_std, double *returns, double *traj, double *moments,
                        int32_t *status, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (n_dir < 0 || H < 0 || dir_begin < 0) return SW_ERR_SIZE;
    if (n_dir == 0) return SW_OK;
    if (!deltas) return SW_ERR_NULL;
    const RolloutArgs a{policy,  deltas, dir_begin, nu, mean, inv_std, /*state0=*/nullptr,
                        returns, traj, /*final_state=*/nullptr, moments, status};
    return launch_rollouts(p, plan_rollouts(p, &FormLaunchers::rollouts, 2 * n_dir, H, traj != nullptr), true,
                           2 * n_dir, H, a, (hipStream_t)stream);
}

// The ARS simulator gate (ars_agent.py:144-157): the 2 n_dir simulator rollouts of sw_ars_rollouts_f64 in
// the form it would pick without trajectories, returns only, the decision fused into the epilogue.
int sw_ars_gate_f64(const sw_params *sim, int64_t dir_begin, int64_t n_dir, int32_t H, const double *policy,
                    const double *deltas, double nu, const double *mean, const double *inv_std,
                    double sim_thresh, int32_t *admit, double *returns, int32_t *status, void *stream)
{
    int rc = check_params(sim);
    if (rc) return rc;
    if (n_dir < 0 || H < 0 || dir_begin < 0) return SW_ERR_SIZE;
    if (n_dir == 0) return SW_OK;
    if (!policy || !deltas || !admit) return SW_ERR_NULL;
    if ((mean == nullptr) != (inv_std == nullptr)) return SW_ERR_NULL;
    const int64_t n_roll = 2 * n_dir;
    const RolloutPlan plan = plan_rollouts(sim, &FormLaunchers::gate, n_roll, H, false);
    const RolloutArgs a{policy,  deltas, dir_begin, nu, mean, inv_std, /*state0=*/nullptr,
                        returns, /*traj=*/nullptr, /*final_state=*/nullptr, /*moments=*/nullptr, status};
    return launchers(plan.form).gate(sim, plan, n_roll, H, a, sim_thresh, admit, (hipStream_t)stream);
}

// The ARS rollouts of n_agent agents in one launch (plan_multi); the pointers come before the agent and direction limits.
int sw_ars_rollouts_multi_f64(const sw_params *p, int64_t n_agent, int64_t n_dir, int32_t H, const double *policy,
                              const double *deltas, double nu, const double *mean, const double *inv_std,
                              double *returns, double *moments, int32_t *status, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (n_agent < 1 || n_dir < 1 || H < 0) return SW_ERR_SIZE;   // an empty or negative batch: before the pointers
    if (!policy || !deltas || !returns) return SW_ERR_NULL;
    if ((mean == nullptr) != (inv_std == nullptr)) return SW_ERR_NULL;
    const MultiPlan m = plan_multi(p, &FormLaunchers::multi, n_agent, n_dir, H);
    if (!m.fits) return SW_ERR_SIZE;
    const MultiArgs a{policy, deltas, mean, inv_std, returns, moments, status};
    return launchers(m.plan.form).multi(p, m.plan, n_agent, 2 * n_dir, H, a, nu, (hipStream_t)stream);
}

// The safe half of a batch of agents.  Both entry points choose the form and the grid as sw_ars_rollouts_multi_f64
// does (from the slot count of the whole launch, at the maximum n_dir for the counted rollouts: a form must not
// depend on values the host has not seen).
int sw_ars_gate_multi_f64(const sw_params *base, int64_t n_agent, int64_t n_dir, int32_t H, const double *policy,
                          const double *deltas, double nu, const double *mean, const double *inv_std,
                          const double *sim, const double *sim_thresh, int32_t *admit, double *returns,
                          int32_t *status, void *stream)
{
    int rc = check_params(base);
    if (rc) return rc;
    const MultiPlan m = plan_multi(base, &FormLaunchers::gate_multi, n_agent, n_dir, H);
    if (!m.fits) return SW_ERR_SIZE;
    if (!policy || !deltas || !sim || !sim_thresh || !admit || !returns) return SW_ERR_NULL;
    if ((mean == nullptr) != (inv_std == nullptr)) return SW_ERR_NULL;
    const SafeMultiArgs a{policy, deltas, mean, inv_std, returns, /*moments=*/nullptr, status, sim, sim_thresh, admit,
                          /*count=*/nullptr};
    return launchers(m.plan.form).gate_multi(base, m.plan, n_agent, 2 * n_dir, H, a, nu, (hipStream_t)stream);
}

// The gate in an ensemble of simulators: the member launch (the form and the grid of sw_ars_gate_multi_f64 for
// n_agent * n_sim agents), then the fold.  Both on `stream`, nothing in between.
int sw_ars_gate_ensemble_f64(const sw_params *base, int64_t n_agent, int64_t n_sim, int64_t n_dir, int32_t H,
                             const double *policy, const double *deltas, double nu, const double *mean,
                             const double *inv_std, const double *sim, const double *sim_thresh, int32_t *admit,
                             double *worst, int32_t *status, double *member_returns, int32_t *member_status,
                             int32_t *member_admit, void *stream)
{
    int rc = check_params(base);
    if (rc) return rc;
    if (n_agent < 1 || n_sim < 1 || n_agent > 65535 || n_sim > 65535) return SW_ERR_SIZE;   // the product cannot overflow
    const int64_t n_member = n_agent * n_sim;
    const MultiPlan m = plan_multi(base, &FormLaunchers::gate_ensemble, n_member, n_dir, H);
    if (!m.fits) return SW_ERR_SIZE;
    if (!policy || !deltas || !sim || !sim_thresh || !admit || !worst || !member_returns || !member_status ||
        !member_admit)
        return SW_ERR_NULL;
    if ((mean == nullptr) != (inv_std == nullptr)) return SW_ERR_NULL;
    const EnsembleArgs a{policy, deltas, mean, inv_std, member_returns, member_status, sim, sim_thresh, member_admit,
                         (int32_t)n_sim};
    rc = launchers(m.plan.form).gate_ensemble(base, m.plan, n_member, 2 * n_dir, H, a, nu, (hipStream_t)stream);
    if (rc) return rc;
    // fewer threads than the member launch has (one per direction against two rollouts per direction and member)
    const int64_t n_pair = n_agent * n_dir;
    hipLaunchKernelGGL(ars_gate_fold_kernel, dim3((unsigned)((n_pair + kFoldBlock - 1) / kFoldBlock)), dim3(kFoldBlock),
                       0, (hipStream_t)stream, n_pair, n_dir, (int32_t)n_sim, member_returns, member_status,
                       member_admit, admit, worst, status);
    return launch_status();
}

int sw_ars_rollouts_multi_counted_f64(const sw_params *p, int64_t n_agent, int64_t n_dir, const int32_t *count,
                                      int32_t H, const double *policy, const double *deltas, double nu,
                                      const double *mean, const double *inv_std, double *returns, double *moments,
                                      int32_t *status, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    const MultiPlan m = plan_multi(p, &FormLaunchers::counted, n_agent, n_dir, H);
    if (!m.fits) return SW_ERR_SIZE;
    if (!count || !policy || !deltas || !returns) return SW_ERR_NULL;
    if ((mean == nullptr) != (inv_std == nullptr)) return SW_ERR_NULL;
    const SafeMultiArgs a{policy, deltas, mean, inv_std, returns, moments, status, /*sim=*/nullptr,
                          /*sim_thresh=*/nullptr, /*admit=*/nullptr, count};
    return launchers(m.plan.form).counted(p, m.plan, n_agent, 2 * n_dir, H, a, nu, (hipStream_t)stream);
}

// The exploration rollouts of a batch of Basic_ARS / Safe_ARS agents (safe_ars/experiment.py): the form and the grid
// as sw_ars_rollouts_multi_f64 chooses them, with two forms to choose from -- mirror-quad where the plan says so
// (n = 3), one rollout per lane everywhere else (plan_rollouts' fallback rule).  A cost trace counts as capture.
int sw_safe_ars_rollouts_multi_f64(const sw_params *real, int64_t n_agent, int64_t n_dir, int32_t H,
                                   const double *policy, const double *deltas, double nu, const int32_t *gated,
                                   const double *sim, const double *sim_thresh, const double *real_thresh,
                                   int32_t cost_kind, int32_t cost_index, double *returns, double *cost_trace,
                                   double *cost_max, int32_t *first_refused, int32_t *violations, int32_t *status,
                                   void *stream)
{
    int rc = check_params(real);
    if (rc) return rc;
    const MultiPlan m = plan_multi(real, &FormLaunchers::safe_ars_multi, n_agent, n_dir, H, cost_trace != nullptr);
    if (!m.in_range) return SW_ERR_SIZE;
    if ((rc = check_cost(real, cost_kind, cost_index)) != SW_OK) return rc;
    if (!policy || !deltas || !gated || !sim || !sim_thresh || !real_thresh || !returns) return SW_ERR_NULL;
    if (!m.fits) return SW_ERR_SIZE;
    const SafeArsMultiArgs a{policy,  deltas,     gated,    sim,           sim_thresh, real_thresh,
                             returns, cost_trace, cost_max, first_refused, violations, status};
    return launchers(m.plan.form).safe_ars_multi(real, m.plan, n_agent, 2 * n_dir, H, a, nu, cost_kind, cost_index,
                                                 (hipStream_t)stream);
}

// ---- ARS iteration pipeline ---------------------------------------------------------
// Host-side enqueue logic of one ARS iteration in native code: the caller's stream (the
// critical path: rollouts -> [all-gather] -> update), a copy stream for the H2D of the deltas,
// and a ring of SW_PIPELINE_SLOTS buffer slots per process.
//
// Measured on MI355X (profiles/), in the order the design reacted to it:
//  * a device-side cross-stream wait in front of the rollout kernel (hipStreamWaitEvent on the
//    H2D copy or on a covariance pass) delays that kernel by 13-18 us even when the awaited
//    work finished long ago -> the critical stream carries NO device-side waits; the ring is
//    deep enough that every dependency completed iterations earlier and the host only confirms;
//  * an event RECORD between two kernels of the critical stream costs ~4 us -> none either:
//    every rollout launch stores its index to a host-visible flag when it starts (SideJob),
//    which tells the host that everything enqueued before it -- the previous update included --
//    has completed;
//  * a covariance pass launched as its own kernel on a side stream costs the concurrent rollout
//    launch ~5 us whatever its size -> the pass over iteration i's trajectories rides along in
//    the rollout launch of iteration i + 1 as extra workgroups (SideJob); the last one owed is
//    flushed by sw_ars_pipeline_sync_cov.
struct sw_ars_pipeline {
    hipStream_t copy = nullptr;
    hipEvent_t h2d_done[SW_PIPELINE_SLOTS] = {};
    bool h2d_valid[SW_PIPELINE_SLOTS] = {};
    uint32_t *flag_host = nullptr, *flag_dev = nullptr;   // progress flag (pinned, mapped)
    uint32_t launches = 0;                                 // rollout launches issued so far
    hipStream_t last_main = nullptr;                       // the stream of the launches so far ...
    bool main_seen = false;                                // ... (may be the null stream)
    int timing = 0;                                        // 0 off, k: time every k-th launch
    int64_t timing_launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timed;  // around the sampled rollout launches
    // covariance pass owed: the trajectories of the latest rollout launch
    const double *cov_traj = nullptr;
    double *cov_acc = nullptr;
    int64_t cov_rolls = 0;
    int32_t cov_H = 0;
    int cov_block = 0;                                     // workgroup size the pass is run with
    sw_params cov_params = {};
};

namespace {

__global__ void flag_kernel(uint32_t *flag, uint32_t value)
{
    __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Spin until the GPU has STARTED rollout launch number `need` (0-based) of this pipeline.
int wait_flag(const sw_ars_pipeline *pl, uint32_t need)
{
    const volatile uint32_t *f = pl->flag_host;
    // Health check of the stream (instead of spinning forever behind a faulted launch) only after 20 ms
    // without progress, then every 20 ms: hipStreamQuery is NOT free for the device -- to learn whether
    // the last kernel is done the runtime enqueues a marker (a barrier packet with a system-scope release)
    // behind it, and the next rollout launch then starts 5.9 us late.  Queried every ~50 us of spinning,
    // as until round 3, that was one marker per iteration: 233.1 -> 227 us per iteration at the headline
    // config (profiles/r03_u_gap_probe.log).
    auto last = std::chrono::steady_clock::now();
    for (int64_t spins = 0;; ++spins) {
        if ((int32_t)(*f - need) >= 0) return SW_OK;
        if ((spins & 0xfff) == 0xfff) {
            const auto now = std::chrono::steady_clock::now();
            if (now - last >= std::chrono::milliseconds(20)) {
                last = now;
                const hipError_t q = hipStreamQuery(pl->last_main);
                if (q == hipSuccess) return ((int32_t)(*f - need) >= 0) ? SW_OK : SW_ERR_LAUNCH;
                if (q != hipErrorNotReady) return SW_ERR_LAUNCH;
            }
        }
        __builtin_ia32_pause();
    }
}

int flush_owed_cov(sw_ars_pipeline *pl, hipStream_t stream)
{
    if (!pl->cov_traj) return SW_OK;
    const int rc = launch_traj_moments(&pl->cov_params, pl->cov_rolls, pl->cov_H, pl->cov_traj,
                                       pl->cov_acc, pl->cov_block, true, stream);
    pl->cov_traj = nullptr;
    return rc;
}

}  // namespace

int sw_ars_pipeline_create(sw_ars_pipeline **out)
{
    if (!out) return SW_ERR_NULL;
    sw_ars_pipeline *pl = new (std::nothrow) sw_ars_pipeline();
    if (!pl) return SW_ERR_LAUNCH;
    const unsigned evf = hipEventDisableTiming;
    // The copy stream is created with the HIGHEST priority the device offers: streams of one
    // priority share a small pool of hardware queues, and a copy stream that lands on the hardware
    // queue of the caller's (normal-priority) stream has its 64 KB H2D queued BEHIND the rollout
    // kernel it is meant to run ahead of -- the host then waits a whole kernel for every copy
    // (measured: the 4th pipeline of a process ran its iterations in 2.15 ms instead of 0.80,
    // profiles/r03_a_outlier_probe.log).  Another priority class is another queue pool.
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    bool ok = hipStreamCreateWithPriority(&pl->copy, hipStreamNonBlocking, prio_greatest) == hipSuccess &&
              hipHostMalloc((void **)&pl->flag_host, 64, hipHostMallocMapped | hipHostMallocCoherent) ==
                  hipSuccess;
    if (ok) {
        *pl->flag_host = 0u;
        ok = hipHostGetDevicePointer((void **)&pl->flag_dev, pl->flag_host, 0) == hipSuccess;
    }
    for (int i = 0; i < SW_PIPELINE_SLOTS && ok; ++i)
        ok = hipEventCreateWithFlags(&pl->h2d_done[i], evf) == hipSuccess;
    if (!ok) {
        sw_ars_pipeline_destroy(pl);
        return SW_ERR_LAUNCH;
    }
    *out = pl;
    return SW_OK;
}

void sw_ars_pipeline_destroy(sw_ars_pipeline *pl)
{
    if (!pl) return;
    if (pl->copy) (void)hipStreamSynchronize(pl->copy);
    if (pl->main_seen) (void)hipStreamSynchronize(pl->last_main);   // kernels still write the flag
    for (auto &e : pl->timed) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    for (int i = 0; i < SW_PIPELINE_SLOTS; ++i)
        if (pl->h2d_done[i]) (void)hipEventDestroy(pl->h2d_done[i]);
    if (pl->copy) (void)hipStreamDestroy(pl->copy);
    if (pl->flag_host) (void)hipHostFree(pl->flag_host);
    delete pl;
}

int sw_ars_pipeline_slots(void) { return SW_PIPELINE_SLOTS; }

// The host may refill deltas_host[slot] once the H2D copy that last read it has completed.
int sw_ars_pipeline_host_slot_wait(sw_ars_pipeline *pl, int slot)
{
    if (!pl) return SW_ERR_NULL;
    if (slot < 0 || slot >= SW_PIPELINE_SLOTS) return SW_ERR_SIZE;
    if (pl->h2d_valid[slot] && hipEventSynchronize(pl->h2d_done[slot]) != hipSuccess)
        return SW_ERR_LAUNCH;
    return SW_OK;
}

// Everything the covariance accumulators are owed is in them when this returns.
int sw_ars_pipeline_sync_cov(sw_ars_pipeline *pl)
{
    if (!pl) return SW_ERR_NULL;
    if (!pl->main_seen) return SW_OK;
    const int rc = flush_owed_cov(pl, pl->last_main);
    if (rc) return rc;
    return hipStreamSynchronize(pl->last_main) == hipSuccess ? SW_OK : SW_ERR_LAUNCH;
}

int sw_ars_pipeline_timing(sw_ars_pipeline *pl, int enable)
{
    if (!pl) return SW_ERR_NULL;
    pl->timing = enable > 0 ? enable : 0;
    pl->timing_launches = 0;
    if (enable) {
        for (auto &e : pl->timed) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
        pl->timed.clear();
    }
    return SW_OK;
}

int sw_ars_pipeline_rollout_ms(sw_ars_pipeline *pl, double *mean_ms, int64_t *launches)
{
    if (!pl || !mean_ms || !launches) return SW_ERR_NULL;
    double tot = 0.0;
    for (auto &e : pl->timed) {
        if (hipEventSynchronize(e.second) != hipSuccess) return SW_ERR_LAUNCH;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.first, e.second) != hipSuccess) return SW_ERR_LAUNCH;
        tot += ms;
    }
    *launches = (int64_t)pl->timed.size();
    *mean_ms = pl->timed.empty() ? 0.0 : tot / (double)pl->timed.size();
    return SW_OK;
}

int sw_ars_pipeline_next_slot(sw_ars_pipeline *pl)
{
    return pl ? (int)(pl->launches % (uint32_t)SW_PIPELINE_SLOTS) : -1;
}

int sw_ars_iteration_rollouts_f64(sw_ars_pipeline *pl, int slot, const sw_params *p,
                                  int64_t n_dir_total, int64_t dir_begin, int64_t n_dir, int32_t H,
                                  const double *deltas_host, double *deltas_dev,
                                  const double *policy, double nu, const double *mean,
                                  const double *inv_std, double *returns, double *traj,
                                  double *moments, double *cov_acc, int32_t *status, void *stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (!pl || !deltas_host || !deltas_dev) return SW_ERR_NULL;
    if (n_dir < 0 || dir_begin < 0 || H < 0 || n_dir_total < dir_begin + n_dir) return SW_ERR_SIZE;
    // The slot is a function of the pipeline's own call count, never of the caller's bookkeeping:
    // call k uses slot k mod SLOTS, and every call counts -- also a rank's call with an empty
    // shard (world > N), which launches nothing but the progress flag.
    const uint32_t k = pl->launches;
    if (slot != (int)(k % (uint32_t)SW_PIPELINE_SLOTS)) return SW_ERR_SIZE;
    if (cov_acc && !traj && n_dir > 0) return SW_ERR_NULL;
    hipStream_t main = (hipStream_t)stream;
    if (pl->main_seen && pl->last_main != main) {
        // the progress flag orders work on ONE stream; a new stream starts from a clean slate
        if (hipStreamSynchronize(pl->last_main) != hipSuccess) return SW_ERR_LAUNCH;
    }
    pl->last_main = main;
    pl->main_seen = true;
    const size_t bytes = (size_t)n_dir_total * (size_t)((p->n - 1) * (2 * p->n + 2)) * sizeof(double);
    // Call k reuses the buffers of call k - SLOTS: its device deltas were last read by update
    // k - SLOTS (done once launch k - SLOTS + 1 has started) and its trajectories by the
    // covariance workgroups of launch k - SLOTS + 1 (done once launch k - SLOTS + 2 has started).
    if (k >= (uint32_t)SW_PIPELINE_SLOTS) {
        rc = wait_flag(pl, k + 2u - (uint32_t)SW_PIPELINE_SLOTS);
        if (rc) return rc;
    }
    if (hipMemcpyAsync(deltas_dev, deltas_host, bytes, hipMemcpyHostToDevice, pl->copy) != hipSuccess)
        return SW_ERR_LAUNCH;
    if (hipEventRecord(pl->h2d_done[slot], pl->copy) != hipSuccess) return SW_ERR_LAUNCH;
    pl->h2d_valid[slot] = true;
    // host-confirmed: the deltas have landed -> the rollout launch needs no device-side wait
    if (hipEventSynchronize(pl->h2d_done[slot]) != hipSuccess) return SW_ERR_LAUNCH;
    if (n_dir == 0) {
        // empty shard: keep the flag sequence going (the host paces the ring on it)
        hipLaunchKernelGGL(flag_kernel, dim3(1), dim3(1), 0, main, pl->flag_dev, k);
        rc = launch_status();
        if (rc) return rc;
        pl->launches = k + 1u;
        return SW_OK;
    }
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    const bool timed_launch = pl->timing > 0 && (pl->timing_launches++ % pl->timing) == 0;
    if (timed_launch) {
        if (hipEventCreate(&ev.first) != hipSuccess || hipEventCreate(&ev.second) != hipSuccess ||
            hipEventRecord(ev.first, main) != hipSuccess)
            return SW_ERR_LAUNCH;
    }
    // ONE plan for the ride-along decision below and for the launch itself
    const RolloutPlan plan = plan_rollouts(p, &FormLaunchers::rollouts, 2 * n_dir, H, traj != nullptr);
    const int cov_block = owed_cov_block(plan.form);
    SideWork sj{pl->flag_dev, k, nullptr, nullptr, 0, 0};
    // the owed pass rides along when this launch's kernel can carry it in the tiling it is owed in
    const bool ride = pl->cov_traj && plan.carries_side && pl->cov_params.n == p->n &&
                      pl->cov_block == cov_block;
    if (pl->cov_traj && !ride) {
        rc = flush_owed_cov(pl, main);
        if (rc) return rc;
    }
    if (ride) {
        sj.cov_traj = pl->cov_traj;
        sj.cov_acc = pl->cov_acc;
        sj.cov_rolls = pl->cov_rolls;
        sj.cov_H = pl->cov_H;
    }
    if (!plan.carries_side) {
        // the lane kernel takes no side job: the flag as a launch of its own in front of it
        hipLaunchKernelGGL(flag_kernel, dim3(1), dim3(1), 0, main, pl->flag_dev, k);
        rc = launch_status();   // a failed flag launch must surface here, not iterations later in wait_flag
        if (rc) return rc;
    }
    const RolloutArgs a{policy,  deltas_dev, dir_begin, nu, mean, inv_std, /*state0=*/nullptr,
                        returns, traj, /*final_state=*/nullptr, moments, status};
    rc = launch_rollouts(p, plan, true, 2 * n_dir, H, a, main, &sj);
    if (timed_launch) {
        (void)hipEventRecord(ev.second, main);
        pl->timed.push_back(ev);
    }
    if (rc) return rc;
    if (ride) pl->cov_traj = nullptr;   // rode along in this launch
    pl->launches = k + 1u;
    // this launch's trajectories are owed a covariance pass: the next launch carries it
    if (cov_acc) {
        pl->cov_traj = traj;
        pl->cov_acc = cov_acc;
        pl->cov_rolls = 2 * n_dir;
        pl->cov_H = H;
        pl->cov_block = cov_block;
        pl->cov_params = *p;
    }
    return SW_OK;
}

int sw_ars_iteration_update_f64(sw_ars_pipeline *pl, int slot, const sw_params *p, int64_t n_dir,
                                const double *gathered, int32_t world, int64_t chunk,
                                int64_t rows_chunk, const double *deltas_dev, double *policy,
                                double alpha, double b, int64_t top_b, double *running,
                                int64_t n_new_states, double *mean, double *inv_std,
                                double *sigma_out, void *stream)
{
    if (!pl) return SW_ERR_NULL;
    if (slot < 0 || slot >= SW_PIPELINE_SLOTS) return SW_ERR_SIZE;
    return sw_ars_update_gathered_f64(p, n_dir, gathered, world, chunk, rows_chunk, deltas_dev,
                                      policy, alpha, b, top_b, running, n_new_states, mean,
                                      inv_std, sigma_out, stream);
}

}  // extern "C"
