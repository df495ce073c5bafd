/*
 * swimmer_hip.h -- C ABI of libswimmer_hip.so, the MI355X (gfx950) implementation of the
 * reference's swimmer-physics + ARS-rollout hot path.
 *
 * Every entry point is `extern "C"`, takes plain device pointers and sizes, allocates
 * nothing, keeps no global state, never throws, and is asynchronous on the HIP stream it
 * is given (`stream` is a hipStream_t passed as void*; NULL = the default stream).  All
 * arithmetic is IEEE fp64.  All pointers are DEVICE pointers unless marked "host".
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   sw_step_f64          SwimmerEnv.step -> next_observation -> compute_accelerations ->
 *                        solve, + get_reward     envs/gym_swimmer/swimmer/remy_swimmer_env.py:41-56,
 *                                                :69-93, :95-214, :238-243
 *   sw_accel_f64         SwimmerEnv.compute_accelerations           remy_swimmer_env.py:95-114
 *   sw_reset_f64         SwimmerEnv.reset                           remy_swimmer_env.py:58-67
 *   sw_rollout_f64       Environment.select_action + .rollout       ars/environment.py:19-57
 *   sw_ars_rollouts_f64  ARSAgent.runOneIteration's perturb + 2N rollouts loop
 *                                                                   ars/ars_agent.py:137-172
 *   sw_ars_gate_f64      ARSAgent.runOneIteration's simulator gate (safe=True): both simulator
 *                        rollouts of every direction + the admit decision
 *                                                                   ars/ars_agent.py:144-157
 *   sw_ars_update_f64    ARSAgent.sort_directions / update_policy and the V2 statistics
 *                                                                   ars/ars_agent.py:97-130, :176-182
 *   sw_ars_rollouts_multi_f64, sw_ars_update_multi_f64
 *                        the same two for every seed of Experiment.plot at once (one Ray actor per seed in the
 *                        reference)                                  ars/experiment.py:61-72
 *   sw_ars_gate_multi_f64, sw_ars_pack_admitted_f64, sw_ars_rollouts_multi_counted_f64,
 *   sw_ars_update_multi_counted_f64
 *                        the safe iteration (ars_agent.py:137-184) for every agent of ars/safe_exploration.py's sweep
 *                        at once (one Ray actor per agent in the reference)   ars/safe_exploration.py
 *   sw_ars_gate_ensemble_f64
 *                        the simulator threshold the reference leaves open (`# TODO compute sim_threshold`): the gate
 *                        in an ensemble of simulators, a direction admitted only where every one admits it
 *                                                                   ars/ars_agent.py:64-72, :144-157
 *   sw_traj_moments_f64  np.mean / np.cov over the saved states     ars/ars_agent.py:180-182
 *   sw_env1_step         the same step for ONE swimmer handed over in host memory (the Gym
 *                        surface and the RL-Glue env_step, SwimmerEnvironment.cpp:53-68)
 *   sw_step_residual_f64 Estimator.I: every stored transition re-simulated and compared with its stored next
 *                        state                                       ars/estimator.py:36-62
 *   sw_step_residual_pop_f64  Estimator.I for a whole CMA-ES generation in one launch (the objective of
 *                        Estimator.estimate_real_env_param's search)  ars/estimator.py:36-62, :89-110
 *   sw_step_residual_sets_f64, sw_step_residual_normal_sets_f64
 *                        the same search, and its least-squares refinement, for many estimators in lock-step: one
 *                        launch per generation / per refinement request for all of them (ars/estimator_batch.py)
 *   sw_safe_rollouts_f64 Safe_ARS.isSafe + Safe_ARS.rollout (the one-step simulator look-ahead that gates
 *                        every real step)                            safe_ars/ars.py:111-153
 *   sw_safe_ars_rollouts_multi_f64
 *                        Basic_ARS.rollout / Safe_ARS.rollout for the 2N perturbed policies of every agent of
 *                        safe_ars/experiment.py at once                safe_ars/ars.py:20-31, :111-153, :84-94
 *   sw_safe_ars_rollouts_ensemble_f64  the same with the per-step gate in an ensemble of up to 64 simulators per agent
 *                        (where the script has `sim_thresh = thresh - 1`)   safe_ars/experiment.py:59
 *   sw_cacla_run_f64     CACLA_agent.run with TwoLayersNet / ActorFA / CriticFA, for every agent of the
 *                        hyper-parameter grid at once   cacla/cacla_agent.py:19-58, :135-199, cacla/swimmer_experiment.py:21-57
 *   sw_cacla_safe_run_f64  the same learner behind the simulator gate of the safe agents (the combination the
 *                        reference does not have)   cacla/cacla_safe_agent.py:161-188, safe_ars/ars.py:111-122
 *   sw_cacla_safe_ensemble_run_f64  the same with the gate in an ensemble of up to 64 simulators per agent (where the
 *                        reference leaves `# TODO compute sim_threshold`)   ars/ars_agent.py:59-70
 *   sw_lqr_cacla_run_f64 CACLA_LQR_agent.run and the safe agents' run loops on the LQR environments, one agent per
 *                        lane   cacla/cacla_agent.py:202-297, cacla/cacla_safe_agent.py, envs/gym_lqr/lqr_env.py
 *   sw_rlglue_ars_run_f64  SwimmerARSAgent under SwimmerExperiment's loop on the native swimmer, one agent per
 *                        lane   rlglue/agent/SwimmerAgent.py:61-239, rlglue/experiment/SwimmerExperiment.cpp:65-84
 *
 * Layouts (d = 2n+2 observation size, m = n-1 action size):
 *   state, SoA    [d][n_env]   field-major: row f holds field f of every env; fields are
 *                              the reference's observation order [Gdx, Gdy, th1, thd1, ...,
 *                              thn, thdn] (remy_swimmer_env.py:216-224).  Coalesced: lane e
 *                              of a wave reads element e of each row.
 *   action, SoA   [m][n_env]
 *   policies, AoS [n_roll][m][d]   exactly numpy's np.array(list_of_(m,d)_matrices)
 *   deltas,  AoS  [n_dir][m][d]    ars_agent.py:137-138
 *   traj          [H][d][n_roll]   step-major, then field, then rollout (coalesced stores);
 *                                  the reference's trajectories[r][t][f] is traj[t][f][r]
 *   returns       [n_roll];  for the ARS entry point rollout 2i is P+nu*delta_i and 2i+1 is
 *                            P-nu*delta_i, the reference's `rewards` order (ars_agent.py:161-169)
 */
#ifndef SWIMMER_HIP_H
#define SWIMMER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SW_ABI_VERSION 3
#define SW_MAX_SEGMENTS 8 /* kernels are instantiated for n = 2..8 */

/* status codes (return values) */
#define SW_OK 0
#define SW_ERR_NULL 1        /* a required pointer is NULL */
#define SW_ERR_SEGMENTS 2    /* n outside 2..SW_MAX_SEGMENTS */
#define SW_ERR_SIZE 3        /* negative / zero size where not allowed */
#define SW_ERR_PARAM 4       /* non-finite or non-positive l_i / m_i, non-finite k / h */
#define SW_ERR_LAUNCH 5      /* hipLaunch failed; see hipGetLastError on the caller side */

/* per-env / per-rollout status bits written to the optional `status` arrays */
#define SW_STATUS_OK 0
#define SW_STATUS_SINGULAR 1 /* a pivot of the joint-acceleration system was <= 0 or not
                                finite: numpy.linalg.solve would raise LinAlgError
                                (remy_swimmer_env.py:212) */
#define SW_STATUS_NONFINITE 2 /* the new state contains inf / nan */
#define SW_STATUS_RANGE 4     /* an angle reached |theta| >= 3e9 rad, outside the range of the
                                 in-kernel sin/cos: outputs are NaN (a simulation that far gone
                                 has ulp(theta) > 4e-7 rad and no meaning left) */
#define SW_STATUS_PARAM 8     /* sw_step_residual_pop_f64: this candidate's l_i / m_i is non-positive or not
                                 finite, or its k is not finite (the rule behind SW_ERR_PARAM): its
                                 partials and value are NaN, the other candidates are unaffected */

/* sw_params.flags: force one of the two rollout kernels (default: chosen from n and n_roll).
 * Both compute the same rollouts; they differ in summation order only (a few ulp per step). */
#define SW_FLAG_ROLLOUT_LANE 1 /* one rollout per lane (throughput form, any n) */
#define SW_FLAG_ROLLOUT_QUAD 2 /* one segment per lane (latency form): a DPP quad per rollout for
                                  n = 3, a 16-lane DPP row per rollout for n = 4..8; n = 2 ignores it */

/* sw_params.flags: n = 3 rollouts with trajectory capture AND V2 moments record a step with one wave-wide store and
 * one moment pair (all eight state components of a rollout on its eight lanes).  This bit keeps them on the kernel
 * that records with three partly masked stores and six sums instead.  Same outputs bit for bit; for A/B measurements
 * and for tests.  Launches without capture or without moments ignore it. */
#define SW_FLAG_CAPTURE_SPLIT 8
/* The same launches record in the packed form through a kernel with a leaner step (store offsets in loop-invariant
 * scalar registers, range test on vcc).  This bit keeps them on the first packed kernel.  Same outputs bit for bit;
 * for A/B measurements and for tests.  Together with SW_FLAG_CAPTURE_SPLIT it is SW_ERR_PARAM. */
#define SW_FLAG_CAPTURE_PACKED_V1 16
/* The same launches take one entry of a lane's 3x3 system from the neighbouring lane instead of forming it a second
 * time (three f64 instructions fewer per step).  This bit keeps them on the lean-step kernel before that.  Same outputs
 * bit for bit; for A/B measurements and for tests.  Together with SW_FLAG_CAPTURE_SPLIT or SW_FLAG_CAPTURE_PACKED_V1
 * it is SW_ERR_PARAM.  (32 and 64 are not flags.) */
#define SW_FLAG_CAPTURE_LEAN_V1 128

/* sw_params.flags: which of the reference's two swimmer models the kernels integrate.
 * Default (bit clear): the Gym env (envs/gym_swimmer/swimmer/remy_swimmer_env.py, explicit
 * Euler, reset = (0, 0, pi/2, 0, ...)).  Bit set: the native RL-Glue environment
 * (rlglue/environment/SwimmerEnvironment.cpp:102-277: its (5n+2)-unknown formulation with
 * its quirks, semi-implicit Euler, start state = all 0.001) -- a different numerical model
 * (they give different accelerations for the same state).  Rollouts of the twin model run on
 * the lane-per-rollout kernel. */
#define SW_FLAG_MODEL_TWIN 4

/* Physical parameters of one swimmer model: SwimmerEnv.__init__ (remy_swimmer_env.py:16-39).
 * max_u is not here: the reference never enforces it (actions are not clipped).  (Its RL-Glue agent does clip:
 * sw_rlglue_ars_run_f64 takes max_u as an argument.) */
typedef struct sw_params {
    int32_t n;        /* segments */
    int32_t flags;    /* 0, or SW_FLAG_* bits (rollout kernel choice, model choice) */
    double l_i;       /* segment length */
    double m_i;       /* segment mass */
    double k;         /* viscous friction coefficient */
    double h;         /* explicit-Euler time step */
    double dir_x;     /* reward = Gdot_new . direction */
    double dir_y;
} sw_params;

int sw_abi_version(void);
const char *sw_strerror(int code);
int sw_max_segments(void);

/* state[f][e] <- reset state (Gdot = 0, theta = pi/2, thetadot = 0). */
int sw_reset_f64(const sw_params *p, int64_t n_env, double *state, void *stream);

/* One physics step for n_env independent swimmers.  state_out may alias state_in.
 * reward and status may be NULL. */
int sw_step_f64(const sw_params *p, int64_t n_env, const double *state_in,
                const double *action, double *state_out, double *reward,
                int32_t *status, void *stream);

/* Accelerations only: gdd [2][n_env], tdd [n][n_env]. */
/* The estimator's objective in one pass (ars/estimator.py:36-62): for every stored transition (state, action,
 * stored next state; SoA like sw_step_f64) the Euclidean distance || step(state, action) - next_ref ||_2, summed in a
 * fixed order per workgroup: partial[b] = sum over transitions [b * B, (b + 1) * B), B = n_env / sw_step_residual_blocks
 * rounded up to the workgroup size (256).  I(x) is the sum of `partial` (sw_step_residual_blocks(n_env) doubles).  Nothing
 * else is written: the simulated next states never reach memory.  Gym model only (SW_FLAG_MODEL_TWIN: SW_ERR_PARAM). */
int sw_step_residual_f64(const sw_params *p, int64_t n_env, const double *state, const double *action,
                         const double *next_ref, double *partial, void *stream);
int64_t sw_step_residual_blocks(int64_t n_env);

/* sw_step_residual_f64 for n_cand parameter sets at once, reading each transition once per workgroup for a group of
 * candidates.  cand [n_cand][3] holds each candidate's (l_i, m_i, k); n, h, dir_x, dir_y and flags come from `base`
 * (whose own l_i, m_i, k are validated but not used).  partial [n_cand][sw_step_residual_blocks(n_env)]: row j has
 * the bits sw_step_residual_f64 writes for candidate j.  value [n_cand] (may be NULL): row j of partial summed in one
 * fixed order, bit-reproducible -- lane l of a 64-lane wave adds partial[j][l], partial[j][l + 64], ... in turn from
 * 0.0, then lane sums pair up as in __shfl_down(., 32), (., 16), ..., (., 1).  cand_status [n_cand] (may be NULL):
 * SW_STATUS_PARAM for a candidate that breaks the parameter rule (NaN partials and value), else 0.
 * Errors, before any HIP call: NULL pointer SW_ERR_NULL; n_cand < 1, n_cand > 524280 or n_env < 0 SW_ERR_SIZE;
 * twin model SW_ERR_PARAM.  n_env = 0 writes nothing. */
int sw_step_residual_pop_f64(const sw_params *base, int64_t n_cand, const double *cand, int64_t n_env,
                             const double *state, const double *action, const double *next_ref, double *partial,
                             double *value, int32_t *cand_status, void *stream);

/* sw_step_residual_pop_f64 for candidates that do not all score on the same transitions: a batch of estimators whose
 * searches advance in lock-step, one launch per generation for all of them.
 *   state, action, next_ref : the concatenated transitions of every set, SoA [d][n_env], [m][n_env], [d][n_env]
 *   set_begin [n_set + 1]   : int64, on the device, ascending; set s is columns [set_begin[s], set_begin[s + 1]),
 *                             every set has at least one transition
 *   max_set_len             : the longest set (sizes the grid and the row stride of `partial`)
 *   cand [n_cand][3]        : (l_i, m_i, k) per candidate; cand_set [n_cand]: int32, on the device, ascending (the
 *                             candidates of a set are contiguous); a set may have no candidate
 *   partial [n_cand][sw_step_residual_blocks(max_set_len)] : the first sw_step_residual_blocks(length of j's set)
 *                             entries of row j have the bits sw_step_residual_f64 writes for candidate j on its set
 *                             alone (256-transition blocks counted from the set's first column); the rest of the row
 *                             is not written
 *   value [n_cand] (may be NULL) : the written entries of row j summed in sw_step_residual_pop_f64's order
 *   cand_status [n_cand] (may be NULL) : SW_STATUS_PARAM (NaN partials and value) or 0, per candidate
 * A candidate whose set index or bounds do not fit (index outside [0, n_set), columns outside [0, n_env), empty, or
 * longer than max_set_len) is not scored: nothing is read or written for it but its status.
 * Errors, before any HIP call: NULL pointer SW_ERR_NULL; n_set < 1, n_cand < 1, n_cand > 524280, max_set_len < 1,
 * n_env < 1 or max_set_len > n_env SW_ERR_SIZE; twin model SW_ERR_PARAM. */
int sw_step_residual_sets_f64(const sw_params *base, int64_t n_set, const int64_t *set_begin, int64_t max_set_len,
                              int64_t n_cand, const double *cand, const int32_t *cand_set, int64_t n_env,
                              const double *state, const double *action, const double *next_ref, double *partial,
                              double *value, int32_t *cand_status, void *stream);

/* The normal equations of the estimator's least-squares refinement, per transition set, fused: every transition of set
 * s is stepped at n_point parameter points, points [n_set][n_point][3] = (l_i, m_i, k), and the residual vectors r =
 * step - next_ref (d components) are reduced without reaching memory.
 *   n_point = 1 : out [n_set][1]  = r.r
 *   n_point = 7 : points in the order centre, +e0, -e0, +e1, -e1, +e2, -e2; J_i = (r_{+i} - r_{-i}) inv_2e[s][i]
 *                 (inv_2e [n_set][3]); out [n_set][13] = r.r | J^T J (9, row-major, symmetric in its bits) | J^T r (3),
 *                 r at the centre
 *   partial [n_set][1 or 13][sw_step_residual_blocks(max_set_len)] : scratch, the per-workgroup sums
 *   active [n_set] (int32, may be NULL) : a set with active[s] == 0 is neither read nor written
 *   set_status [n_set] (may be NULL)    : SW_STATUS_PARAM (NaN sums) when a point of the set breaks the parameter rule
 * Sums go in a fixed order (per transition an FMA chain over the d components; per workgroup the lane tree and wave
 * order of sw_step_residual_f64; per set the order of sw_step_residual_pop_f64's value): bit-reproducible.  A
 * transition with an angle out of range makes its set's sums NaN.  set_begin, max_set_len and the transitions as in
 * sw_step_residual_sets_f64; a set whose bounds do not fit is skipped.
 * Errors, before any HIP call: NULL pointer SW_ERR_NULL (inv_2e only with 7 points); n_set < 1, n_set > 65535,
 * max_set_len < 1, n_env < 1 or max_set_len > n_env SW_ERR_SIZE; twin model or n_point outside {1, 7} SW_ERR_PARAM. */
int sw_step_residual_normal_sets_f64(const sw_params *base, int64_t n_set, const int64_t *set_begin,
                                     int64_t max_set_len, int32_t n_point, const double *points, const double *inv_2e,
                                     const int32_t *active, int64_t n_env, const double *state, const double *action,
                                     const double *next_ref, double *partial, double *out, int32_t *set_status,
                                     void *stream);

int sw_accel_f64(const sw_params *p, int64_t n_env, const double *state,
                 const double *action, double *gdd, double *tdd, void *stream);

/* n_roll independent H-step rollouts of a linear policy, one policy per rollout.
 *   mean, inv_std : [d] each, both NULL -> ARS V1 action a = P s; both given -> V2 action
 *                   a = (P diag(inv_std)) (s - mean), inv_std = diag(cov) ** -0.5
 *   state0        : [d][n_roll] start states, NULL -> reset state
 *   returns       : [n_roll] sum of the H rewards
 *   traj          : NULL or [H][d][n_roll], every post-step state
 *   final_state   : NULL or [d][n_roll]
 *   moments       : NULL or [sw_moments_blocks(n_roll)][2d] partial sums, one row per 16
 *                   consecutive rollouts, of sum(s - c) and sum((s - c)^2) over all their
 *                   post-step states, c = reset state
 *   status        : NULL or [n_roll] */
int sw_rollout_f64(const sw_params *p, int64_t n_roll, int32_t H, const double *policies,
                   const double *mean, const double *inv_std, const double *state0,
                   double *returns, double *traj, double *final_state, double *moments,
                   int32_t *status, void *stream);

/* Safe exploration, safe_ars/ars.py Safe_ARS.rollout (:124-153): n_roll rollouts of H steps from the reset state,
 * every real step gated by a one-step look-ahead in a simulator -- isSafe (:111-122) = one step of the swimmer with
 * the parameters `sim` from the real state under the proposed action policy @ obs (:139), and
 * cost(simulated observation) <= sim_thresh.  A refused step leaves the state where it is (:150-151; the rollout
 * then stays refused: it proposes the same action again).  `real` and `sim` must have the same number of segments;
 * the model flag of `real` / `sim` is ignored (Gym model).  The whole loop is ONE launch: n = 3 up to 8192 rollouts in the
 * mirror-quad form (the look-ahead and the real step share the step's geometry), n = 4..8 in the row form while SIMDs are
 * idle, one rollout per lane otherwise (or with SW_FLAG_ROLLOUT_LANE in real->flags); same results to rounding.
 *   policies      : [n_roll][m][d]
 *   cost_kind     : SW_COST_ABS_OBS            cost = |obs[cost_index]|, obs = [Gdx, Gdy, th_1, thd_1, ...]
 *                   SW_COST_MAX_ABS_THETADOT   cost = max_i |thetadot_i|  (safe_ars/experiment.py:45; cost_index unused)
 *   returns       : [n_roll] sum of the rewards of the steps taken
 *   traj          : NULL or [H][d][n_roll]: the state after step t, the unchanged state where step t was refused
 *   first_refused : NULL or [n_roll]: the first refused step (H: none)
 *   violations    : NULL or [n_roll]: real steps whose cost exceeded real_thresh (the reference prints each, :143-144)
 *   status        : NULL or [n_roll] */
#define SW_COST_ABS_OBS 0
#define SW_COST_MAX_ABS_THETADOT 1
int sw_safe_rollouts_f64(const sw_params *real, const sw_params *sim, int64_t n_roll, int32_t H,
                         const double *policies, int32_t cost_kind, int32_t cost_index, double sim_thresh,
                         double real_thresh, double *returns, double *traj, int32_t *first_refused,
                         int32_t *violations, int32_t *status, void *stream);

/* Number of partial-moment rows sw_rollout_f64 / sw_ars_rollouts_f64 write for n_roll
 * rollouts (= ceil(n_roll / 16), whichever kernel runs). */
int64_t sw_moments_blocks(int64_t n_roll);

/* The ARS exploration batch: for directions i in [dir_begin, dir_begin + n_dir) run the two
 * rollouts P + nu*delta_i and P - nu*delta_i (perturbation fused into the kernel prologue).
 *   policy  : [m][d]          deltas : [>= dir_begin + n_dir][m][d]
 *   returns : [2 * n_dir] local slice, entry 2j / 2j+1 = +/- rollout of direction dir_begin+j
 *   traj    : NULL or [H][d][2 * n_dir];  moments as in sw_rollout_f64 with n_roll = 2 n_dir */
int sw_ars_rollouts_f64(const sw_params *p, int64_t dir_begin, int64_t n_dir, int32_t H,
                        const double *policy, const double *deltas, double nu,
                        const double *mean, const double *inv_std, double *returns,
                        double *traj, double *moments, int32_t *status, void *stream);

/* The safe-ARS simulator gate (ars_agent.py:144-157).  For directions i in [dir_begin, dir_begin + n_dir)
 * run the rollouts P + nu*delta_i and P - nu*delta_i in the simulator `sim` from the reset state, whitened
 * with mean / inv_std exactly as sw_ars_rollouts_f64 does (both NULL for V1), and decide in the same launch
 *   admit[j] = !(r_j+ <= sim_thresh) && !(r_j- <= sim_thresh)        (j = i - dir_begin)
 * the reference's rule: a return equal to the threshold refuses; a NaN return or a NaN threshold admits
 * (x <= NaN is false and the reference then takes the real rollout).  Computing r_j- also when r_j+
 * already refuses is equivalent: the reference's skipped rollout has no side effect.
 * Stores no trajectories and no moments.  The kernel form is the one sw_ars_rollouts_f64 picks without
 * trajectories (mirror-quad / quad for n = 3, row for n = 4..8, lane otherwise; SW_FLAG_ROLLOUT_* honoured).
 *   admit   : [n_dir], required          returns : NULL or [2 * n_dir], as sw_ars_rollouts_f64's
 *   status  : NULL or [2 * n_dir], as sw_ars_rollouts_f64's */
int sw_ars_gate_f64(const sw_params *sim, int64_t dir_begin, int64_t n_dir, int32_t H,
                    const double *policy, const double *deltas, double nu,
                    const double *mean, const double *inv_std, double sim_thresh,
                    int32_t *admit, double *returns, int32_t *status, void *stream);

/* ARS policy update + V2 statistics.
 *   returns       : [2 * n_dir] all returns of the iteration (after the all-gather)
 *   policy        : [m][d], updated in place:
 *                   P += alpha / (div * sigma_R) * sum_{i in used}(r_i+ - r_i-) delta_i
 *                   sigma_R = population std (ddof = 0) of the used returns.
 *   top_b         : 0 -> ars/ars_agent.py's behaviour: every direction is used, b is only a
 *                   divisor (ars_agent.py:176-177, :126-128);  > 0 -> safe_ars/ars.py's
 *                   Basic_ARS: only the top_b directions by max(r+, r-) are used (:95-96),
 *                   sigma_R is taken over their returns (:60) and the divisor is the NUMBER OF
 *                   DIRECTIONS USED, len(order) = min(top_b, n_dir) (:64) -- `b` is ignored
 *   moments       : NULL (V1) or [n_moment_rows][2d] partial sums of this iteration
 *   running       : NULL (V1) or [1 + 2d] statistics of every state since training began
 *                   (ars_agent.py:171, :180: never cleared): {count n, mean - c (d),
 *                   M2 = sum (s - mean)^2 (d)}, c = reset state; zero before the first call.
 *                   Each iteration's batch is merged in (Chan et al. pairwise update): no
 *                   cancellation that grows with the length of training
 *   n_new_states  : states added this iteration (2 * n_dir * H over all ranks)
 *   mean, inv_std : NULL (V1) or [d] each, overwritten with the new mean and
 *                   var ** -0.5 (var with ddof = 1, np.cov's default)
 *   sigma_out     : NULL or [1] */
int sw_ars_update_f64(const sw_params *p, int64_t n_dir, const double *returns,
                      const double *deltas, double *policy, double alpha, double b,
                      int64_t top_b, const double *moments, int64_t n_moment_rows,
                      double *running, int64_t n_new_states, double *mean, double *inv_std,
                      double *sigma_out, void *stream);

/* ---- many agents in lock-step: one rollout launch and one update launch per iteration for ALL of them ----
 * A learning curve is n_seed independent ARSAgents (ars/experiment.py:61-72, one Ray actor per seed).  With the
 * reference's N = 1 .. a handful of directions one agent's iteration is a launch that leaves the chip idle, and the
 * launches of different seeds are independent: these two entry points run them as one.
 *
 * sw_ars_rollouts_multi_f64: sw_ars_rollouts_f64 (dir_begin = 0, no trajectories) for n_agent agents that share
 * p, n_dir, H and nu.  Every array is the single-agent array once per agent, agent-major and dense:
 *   policy  : [n_agent][m][d]             deltas : [n_agent][n_dir][m][d]
 *   mean, inv_std : [n_agent][d] each, or both NULL (V1)
 *   returns : [n_agent][2 * n_dir]        entry 2j / 2j+1 of agent a = +/- rollout of ITS direction j
 *   moments : NULL or [n_agent][sw_moments_blocks(2 * n_dir)][2d]; row i of agent a covers ITS rollouts
 *             16i .. 16i+15, as in a single-agent launch: no row holds states of two agents
 *   status  : NULL or [n_agent][2 * n_dir]
 * Agent a's rollouts read agent a's policy, deltas, mean and inv_std only.  Inside the launch every agent's
 * rollouts are padded to whole workgroups (16 rollout slots, 64 in the lane form); padding slots write nothing.
 * The kernel form is chosen as sw_ars_rollouts_f64 chooses it, from n_agent * 16 * ceil(2 n_dir / 16) slots
 * (SW_FLAG_ROLLOUT_* honoured); per rollout each form runs the instructions of its single-agent kernel, so a
 * launch gives, agent by agent, the bits of sw_ars_rollouts_f64 in the same form.
 * Errors, before any HIP call: NULL policy / deltas / returns, or one of mean / inv_std without the other:
 * SW_ERR_NULL; n_agent < 1, n_dir < 1, H < 0, n_agent > 65535, n_dir > 2^23 or 2^32 threads and more: SW_ERR_SIZE;
 * parameters as everywhere. */
int sw_ars_rollouts_multi_f64(const sw_params *p, int64_t n_agent, int64_t n_dir, int32_t H,
                              const double *policy, const double *deltas, double nu,
                              const double *mean, const double *inv_std, double *returns,
                              double *moments, int32_t *status, void *stream);

/* sw_ars_update_f64 for n_agent agents in one launch.  returns [n_agent][2 * n_dir], deltas [n_agent][n_dir][m][d],
 * policy [n_agent][m][d], moments [n_agent][n_moment_rows][2d], running [n_agent][1 + 2d], mean / inv_std
 * [n_agent][d], sigma_out NULL or [n_agent]; alpha, b, top_b and n_new_states hold for every agent.  Each agent's
 * result has the bits of a sw_ars_update_f64 call on its slices (the order of summation depends on n_dir only).
 * Errors as sw_ars_update_f64, and n_agent < 1 or > 65535: SW_ERR_SIZE. */
int sw_ars_update_multi_f64(const sw_params *p, int64_t n_agent, int64_t n_dir, const double *returns,
                            const double *deltas, double *policy, double alpha, double b,
                            int64_t top_b, const double *moments, int64_t n_moment_rows,
                            double *running, int64_t n_new_states, double *mean, double *inv_std,
                            double *sigma_out, void *stream);

/* ---- safe agents in lock-step: gate, pack, counted rollouts, counted update -- four launches per iteration for ALL
 * agents, nothing read by the host in between ----
 * The safe iteration of ARSAgent (ars_agent.py:137-184) is a gate launch, a host read of the admit flags, then rollouts
 * and update over the k admitted directions.  Here k stays on the device: every agent a has its own simulator,
 * simulator threshold and count[a], and row a of every result has the bits of the single-agent sequence
 * sw_ars_gate_f64 -> (pack on the host) -> sw_ars_rollouts_f64 -> sw_ars_update_f64 with n_dir = count[a].
 * Arrays are agent-major and dense as in sw_ars_rollouts_multi_f64; the form and the grid are chosen as there (from
 * n_agent and the MAXIMUM n_dir: whole workgroups per agent, blockIdx.y = agent).
 * Errors of all four, before any HIP call: a NULL required pointer SW_ERR_NULL; n_agent < 1, n_agent > 65535,
 * n_dir < 1 or H < 0 SW_ERR_SIZE; parameters as everywhere.
 *
 * sw_ars_gate_multi_f64: sw_ars_gate_f64 (dir_begin = 0) for n_agent agents in one launch.
 *   base       : n, h, dir_* and flags of every simulator (its own l_i, m_i, k are validated but not used)
 *   sim        : [n_agent][3] each agent's simulator (l_i, m_i, k); the constants are derived in the kernel by the
 *                function the host uses, so they have the host's bits (the convention of sw_step_residual_pop_f64)
 *   sim_thresh : [n_agent]          admit : [n_agent][n_dir]
 *   policy, deltas, mean / inv_std, returns (required here), status (may be NULL): as sw_ars_rollouts_multi_f64
 * An agent whose simulator breaks the parameter rule (SW_ERR_PARAM's) gets SW_STATUS_PARAM in its status entries, NaN
 * returns and admits nothing; the other agents are unaffected. */
int sw_ars_gate_multi_f64(const sw_params *base, int64_t n_agent, int64_t n_dir, int32_t H, const double *policy,
                          const double *deltas, double nu, const double *mean, const double *inv_std,
                          const double *sim, const double *sim_thresh, int32_t *admit, double *returns,
                          int32_t *status, void *stream);

/* admit [n_agent][n_dir] (and, where given, the gate's status [n_agent][2 n_dir]: a direction with a non-zero status
 * on either of its simulator rollouts counts as refused -- its NaN return would have admitted it) ->
 *   count  : int32 [n_agent]          the admitted directions k
 *   order  : int32 [n_agent][n_dir]   their indices in ascending order in entries 0..k-1, -1 behind them
 *   packed : [n_agent][n_dir][m][d]   their deltas in that order in entries 0..k-1; the rest is not written
 * One workgroup per agent; a prefix sum over the flags (ballot and popcount per 64 directions), so the order never
 * depends on timing.  p gives n only. */
int sw_ars_pack_admitted_f64(const sw_params *p, int64_t n_agent, int64_t n_dir, const int32_t *admit,
                             const int32_t *status, const double *deltas, int32_t *count, int32_t *order,
                             double *packed, void *stream);

/* sw_ars_rollouts_multi_f64 with each agent's direction count read from count [n_agent] on the device (values
 * outside 0..n_dir are clamped); n_dir is the maximum and sets the strides of every array.  Agent a runs 2 count[a]
 * rollouts of its first count[a] deltas and writes returns and status entries 0..2 count[a] - 1 and moment rows
 * 0..ceil(2 count[a] / 16) - 1, with the bits of sw_ars_rollouts_f64(n_dir = count[a]) in the same form; everything
 * behind them is left as it was.  Workgroups behind an agent's last rollout return at once. */
int sw_ars_rollouts_multi_counted_f64(const sw_params *p, int64_t n_agent, int64_t n_dir, const int32_t *count,
                                      int32_t H, const double *policy, const double *deltas, double nu,
                                      const double *mean, const double *inv_std, double *returns, double *moments,
                                      int32_t *status, void *stream);

/* sw_ars_update_multi_f64 with per-agent n_dir = count[a], top_b = min(top_b, count[a]), n_new_states =
 * 2 count[a] H and the agent's ceil(2 count[a] / 16) written moment rows; n_dir and n_moment_rows (>=
 * sw_moments_blocks(2 n_dir) with V2) are the maxima and set the strides.  Each agent's result has the bits of
 * sw_ars_update_f64 on its slices with n_dir = count[a].  An agent with count 0 is left untouched: policy, running,
 * mean, inv_std and sigma_out keep their values.  (From 1025 directions on the single-agent update runs in wider
 * workgroups: two launches then, each serving the agents whose count picks its width.) */
int sw_ars_update_multi_counted_f64(const sw_params *p, int64_t n_agent, int64_t n_dir, const int32_t *count,
                                    int32_t H, const double *returns, const double *deltas, double *policy,
                                    double alpha, double b, int64_t top_b, const double *moments,
                                    int64_t n_moment_rows, double *running, double *mean, double *inv_std,
                                    double *sigma_out, void *stream);

/* ---- the gate in an ENSEMBLE of simulators ----
 * sw_ars_gate_ensemble_f64: sw_ars_gate_multi_f64 with n_sim simulators per agent, and the fold over them.  The
 * reference leaves its simulator threshold open (`# TODO compute sim_threshold`, ars_agent.py:70): threshold +
 * alpha(H) epsilon with Lipschitz constants nobody knows.  Here a direction has to pass in EVERY simulator of a set
 * that stands for the uncertainty -- several estimates, or samples on the epsilon-sphere around one -- and the worst
 * simulated return takes the place of alpha epsilon.
 *   base       : n, h, dir_* and flags of every simulator (its own l_i, m_i, k are validated but not used)
 *   policy, deltas, mean / inv_std : per AGENT, as sw_ars_gate_multi_f64; shared by the agent's members, read in place
 *   sim        : [n_agent][n_sim][3] (l_i, m_i, k) of member e of agent a; constants derived in the kernel, host's bits
 *   sim_thresh : [n_agent]
 *   member_returns / member_status : [n_agent][n_sim][2 n_dir]   member_admit : [n_agent][n_sim][n_dir]
 *                member (a, e) has, bit for bit, the returns, status and flags of sw_ars_gate_f64 (dir_begin = 0) in
 *                simulator sim[a][e] against sim_thresh[a] in the same form: member_admit = !(r+ <= thr) &&
 *                !(r- <= thr), equality refuses, a NaN return or threshold admits.  All three are required: the fold
 *                reads them.
 *   admit      : [n_agent][n_dir]    the AND over e of member_admit
 *   worst      : [n_agent][2 n_dir]  the minimum over e of the members' return r, taken as w = (x < w) ? x : w from
 *                +inf in ascending e: a NaN never replaces w, and where every member's return is NaN worst is +inf
 *   status     : NULL or [n_agent][2 n_dir]  the bitwise OR over e of the members' status (SW_STATUS_* are bit flags)
 * A member whose simulator breaks the parameter rule gets SW_STATUS_PARAM, NaN returns and admits nothing (as in
 * sw_ars_gate_multi_f64), so its whole agent admits nothing; the other agents are unaffected.  Where both status
 * entries of a direction are 0, admit == !(worst+ <= thr) && !(worst- <= thr): a return with status 0 is finite, a
 * refusing member holds one <= thr, and the minimum then is too.  admit, worst and status have the layout
 * sw_ars_pack_admitted_f64 reads.
 * Two launches on `stream`: the member kernels on the grid (workgroups of one agent, n_agent * n_sim), form and grid
 * chosen as sw_ars_gate_multi_f64 chooses them for n_agent * n_sim agents (SW_FLAG_ROLLOUT_* and the model flag
 * honoured), then the fold, one thread per (agent, direction), plain loads and stores: no result depends on timing.
 * Errors, before any HIP call: a NULL required pointer, or one of mean / inv_std without the other: SW_ERR_NULL;
 * n_agent < 1, n_sim < 1, n_agent * n_sim > 65535, n_dir < 1, n_dir > 2^23, H < 0 or 2^32 threads and more:
 * SW_ERR_SIZE; parameters as everywhere. */
int sw_ars_gate_ensemble_f64(const sw_params *base, int64_t n_agent, int64_t n_sim, int64_t n_dir, int32_t H,
                             const double *policy, const double *deltas, double nu, const double *mean,
                             const double *inv_std, const double *sim, const double *sim_thresh, int32_t *admit,
                             double *worst, int32_t *status, double *member_returns, int32_t *member_status,
                             int32_t *member_admit, void *stream);

/* ---- safe_ars/experiment.py: Basic_ARS and Safe_ARS agents in lock-step, the per-step gate inside the rollout ----
 * sw_safe_ars_rollouts_multi_f64: the 2 n_dir exploration rollouts of n_agent agents in one launch, every rollout with
 * the semantics of sw_safe_rollouts_f64 -- H steps from the reset state, action policy @ obs (V1), every real step gated
 * by the one-step simulator look-ahead -- with three differences:
 *   - rollout 2j / 2j+1 of agent a runs the policy P_a + / - nu delta_{a,j}, formed in the kernel with the rounding
 *     of sw_ars_rollouts_f64 (NumPy's `P + nu * delta` / `P - nu * delta`, bit for bit);
 *   - the gate is per agent: gated[a] == 0 is Basic_ARS.rollout (safe_ars/ars.py:20-31), every step is taken and the
 *     look-ahead is not computed -- no threshold and no NaN cost stops such a rollout;
 *   - every gated agent has its own simulator and simulator threshold, every agent its own real threshold.
 * No trajectory is stored: the experiment reads its states as cost(state) only (safe_ars/experiment.py:81-82).
 *   real          : the real swimmer (n, l_i, m_i, k, h, dir_*; SW_FLAG_ROLLOUT_* honoured; Gym model)
 *   policy        : [n_agent][m][d]         deltas : [n_agent][n_dir][m][d]
 *   gated         : [n_agent]  0: Basic_ARS.rollout; else Safe_ARS.rollout
 *   sim           : [n_agent][3] (l_i, m_i, k) of each agent's simulator, read for gated agents only; the constants
 *                   are derived in the kernel by the function the host uses (as in sw_ars_gate_multi_f64)
 *   sim_thresh    : [n_agent], read for gated agents only; a NaN refuses step 0 (cost <= NaN is false)
 *   real_thresh   : [n_agent]
 *   cost_kind, cost_index : SW_COST_* as sw_safe_rollouts_f64
 *   returns       : [n_agent][2 n_dir], entry 2j / 2j+1 = rollout of P + / - nu delta_j: the rewards of the steps taken
 *   cost_trace    : NULL or [H][n_agent][2 n_dir]: cost of the state the reference appends to `states` at step t -- the
 *                   state after the step, or the unchanged state where step t was refused (:149-152); NaN propagates
 *                   as in np.max
 *   cost_max      : NULL or [n_agent][2 n_dir]: the maximum of that over t (NaN if any is NaN; 0 for H = 0)
 *   first_refused : NULL or [n_agent][2 n_dir]: the first refused step (H: none; always H for an ungated agent)
 *   violations    : NULL or [n_agent][2 n_dir]: steps taken whose cost exceeded real_thresh, for ungated agents too
 *   status        : NULL or [n_agent][2 n_dir]
 * A gated agent whose simulator breaks the parameter rule (SW_ERR_PARAM's) gets SW_STATUS_PARAM in its status entries,
 * NaN returns (and NaN cost_trace / cost_max entries), first_refused 0 and no violations; the other agents are
 * unaffected.  Two kernel forms, chosen as sw_ars_rollouts_multi_f64 chooses (whole workgroups per agent, blockIdx.y =
 * agent; surplus slots recompute the agent's last rollout and store nothing): n = 3 in the mirror-quad form of
 * sw_safe_rollouts_f64 while SIMDs are idle, one rollout per lane otherwise and for every other n (there is no row
 * form).  Per rollout each form runs the arithmetic of sw_safe_rollouts_f64 in the same form: returns, first_refused,
 * violations and status of a gated agent have its bits, those of an ungated agent the bits of sw_rollout_f64.
 * Errors, before any HIP call: a NULL policy / deltas / gated / sim / sim_thresh / real_thresh / returns: SW_ERR_NULL;
 * n_agent < 1, n_agent > 65535, n_dir < 1, n_dir > 2^23, H < 0, an unknown cost_kind, a cost_index outside 0..d-1 with
 * SW_COST_ABS_OBS, or 2^32 threads and more: SW_ERR_SIZE; parameters as everywhere. */
int sw_safe_ars_rollouts_multi_f64(const sw_params *real, int64_t n_agent, int64_t n_dir, int32_t H,
                                   const double *policy, const double *deltas, double nu, const int32_t *gated,
                                   const double *sim, const double *sim_thresh, const double *real_thresh,
                                   int32_t cost_kind, int32_t cost_index, double *returns, double *cost_trace,
                                   double *cost_max, int32_t *first_refused, int32_t *violations, int32_t *status,
                                   void *stream);

/* ---- the same rollouts, every step of a gated agent gated on an ENSEMBLE of simulators (the per-step side of
 * sw_ars_gate_ensemble_f64 and sw_cacla_safe_ensemble_run_f64: the members stand for the uncertainty about
 * (l_i, m_i, k), where safe_ars/experiment.py:59 has one simulator and `sim_thresh = thresh - 1`) ----
 * sw_safe_ars_rollouts_ensemble_f64: sw_safe_ars_rollouts_multi_f64 with n_member simulators per agent.  Every argument
 * of that function keeps its meaning, layout and NULL rule.  Step t of a rollout of a gated agent:
 *   u = (P +- nu delta) @ obs
 *   c_e = cost(step(obs, u) with member e's constants)     for every member e (n, h, direction are `real`'s)
 *   the step is taken iff c_e <= sim_thresh[a] for EVERY e  (a NaN cost or threshold refuses)
 *   a refused rollout stops stepping and repeats its state, as in sw_safe_ars_rollouts_multi_f64
 * The members ride in lanes: a rollout owns a group of G lanes of a wave, G the smallest power of two >= n_member, lane
 * j with the constants of member j % n_member, and the gate is a wave ballot -- so an agent has at most 64 members:
 * MORE THAN ONE WAVE'S WORTH OF MEMBERS IS NOT BUILT.  One kernel form for every n = 2..8, one rollout group per
 * 64 / G of a 64-thread workgroup, grid (ceil(2 n_dir G / 64), n_agent); SW_FLAG_ROLLOUT_* is accepted and ignored.  A
 * MIRROR-QUAD ENSEMBLE FORM FOR n = 3 AND A ROW FORM ARE NOT BUILT.  The arithmetic is that of the lane form: with
 * n_member = 1, or with n_member copies of one simulator, every output the two functions share has the bits of
 * sw_safe_ars_rollouts_multi_f64 under SW_FLAG_ROLLOUT_LANE in that simulator, and an agent with gated[a] == 0 (which
 * reads neither sims nor sim_thresh) has that function's ungated bits.  The order of an agent's members changes nothing
 * but the order of the bits of refusing_members.
 *   n_member      : 1..64, the same for every agent
 *   sims          : [n_agent][n_member][3] (l_i, m_i, k) of each member, read for gated agents only; the constants are
 *                   derived in the kernel by the function the host uses
 *   worst_max     : NULL or [n_agent][2 n_dir]: the maximum of c_e over the ADMITTED steps and over all e, so never
 *                   above sim_thresh; 0 where no step was admitted (costs are >= 0); NaN for an ungated agent
 *   refusing_members : NULL or [n_agent][2 n_dir]: bit e set iff member e's own cost was not <= sim_thresh at the first
 *                   refused step (which member binds); 0 where no step was refused and for an ungated agent
 * A gated agent with a member that breaks the parameter rule (SW_ERR_PARAM's) gets SW_STATUS_PARAM, NaN returns,
 * cost_trace, cost_max and worst_max, first_refused 0, no violations and the bits of the bad members in
 * refusing_members; the other agents are unaffected.  Only lane 0 of a group stores, with plain stores: no result
 * depends on timing.
 * Errors, before any HIP call: those of sw_safe_ars_rollouts_multi_f64 (worst_max and refusing_members may be NULL);
 * n_member < 1, n_member > 64 or 2^32 threads and more (64 per 64 / G rollouts) SW_ERR_SIZE; twin model SW_ERR_PARAM. */
int sw_safe_ars_rollouts_ensemble_f64(const sw_params *real, int64_t n_agent, int32_t n_member, int64_t n_dir, int32_t H,
                                      const double *policy, const double *deltas, double nu, const int32_t *gated,
                                      const double *sims, const double *sim_thresh, const double *real_thresh,
                                      int32_t cost_kind, int32_t cost_index, double *returns, double *cost_trace,
                                      double *cost_max, int32_t *first_refused, int32_t *violations, int32_t *status,
                                      double *worst_max, int64_t *refusing_members, void *stream);

/* ---- CACLA (cacla/cacla_agent.py): whole training runs of many independent agents in ONE launch ----
 * An agent is n networks -- the n - 1 actors of ActorFA (one per torque), then the critic of CriticFA -- each a
 * TwoLayersNet(d, SW_CACLA_HIDDEN): linear1 (d -> 12), relu, linear2 (12 -> 1), fp64.  One network is
 * SW_CACLA_NET_DOUBLES(n) doubles:
 *   W1 [12][d] row-major (linear1.weight) | b1 [12] (linear1.bias) | W2 [12] (linear2.weight) | b2 (linear2.bias)
 * sw_cacla_run_f64 runs n_iter steps of CACLA_agent.run (cacla_agent.py:170-193) for n_agent agents, one wave each:
 *   train != 0: FA_act = actors(state); action = FA_act + noise[t]; new_state, reward = step(action);
 *               temp_diff = reward + gamma V(new_state) - V(state); critic += alpha temp_diff dV/dw at `state`;
 *               if temp_diff > 0: actor_i += alpha (action_i - FA_act_i) dA_i/dw at `state`; state = new_state
 *   train == 0: the reference as written (:173-178): no updates, and the actors see the state THE CALL STARTED
 *               FROM at every step while the swimmer keeps stepping (so a split run is not one run); weights are
 *               not written
 * No action clipping, no reset, `done` ignored.  Arithmetic is not trapped: NaN propagates into the rewards (the
 * reference takes np.nanmean over seeds) and a NaN temp_diff skips the actor update.
 *   gamma, alpha  : [n_agent]
 *   noise         : [n_agent][n_iter][n-1], added to the actors' outputs: the caller's N(0, sigma) draws
 *   weights       : in/out [n_agent][n][SW_CACLA_NET_DOUBLES(n)]
 *   state         : in/out [n_agent][d], AoS: one agent's observation is contiguous; out = the swimmer's state
 *   rewards       : [n_agent][n_iter]
 *   actor_updates : NULL or [n_agent], += the steps with temp_diff > 0
 *   status        : NULL or [n_agent], |= SW_STATUS_SINGULAR / NONFINITE (state after the call) / RANGE; zero it
 *                   before the first call of a run
 * weights and state are in/out so that a run can be split into launches: the split changes no bit (train != 0).
 * Errors, before any HIP call: NULL pointer SW_ERR_NULL; n_agent < 1, n_agent > 2^31 - 1 or n_iter < 0 SW_ERR_SIZE;
 * twin model SW_ERR_PARAM; n outside 2..8 SW_ERR_SEGMENTS.  n_iter = 0 writes nothing. */
#define SW_CACLA_HIDDEN 12 /* cacla_agent.py:165-166 */
#define SW_CACLA_NET_DOUBLES(n) (SW_CACLA_HIDDEN * (2 * (n) + 2) + 2 * SW_CACLA_HIDDEN + 1)
int sw_cacla_run_f64(const sw_params *p, int64_t n_agent, int32_t n_iter, int32_t train,
                     const double *gamma, const double *alpha, const double *noise, double *weights,
                     double *state, double *rewards, int32_t *actor_updates, int32_t *status, void *stream);

/* ---- CACLA on the swimmer with safe exploration: the learner above inside the run loop of the reference's safe
 * agents (cacla/cacla_safe_agent.py:161-188, LQR-only there), every real step gated by a one-step look-ahead in the
 * agent's simulator (safe_ars/ars.py:111-122) ----
 * sw_cacla_safe_run_f64 runs n_iter steps for n_agent agents, one wave each, always training.  Step t of a gated agent:
 *   FA_act = actors(state); action = FA_act + noise[t]   (the noise of step t is consumed whether or not it is taken)
 *   sim_state = step(state, action) with the agent's simulator constants (n, h and direction are `real`'s)
 *   admitted = cost(sim_state) <= sim_thresh[a]           (a NaN cost or threshold refuses)
 *   admitted: new_state, reward = the real step; violations += cost(new_state) > real_thresh[a] (false for NaN);
 *             temp_diff, the critic's update and -- when temp_diff > 0 -- the actors' as sw_cacla_run_f64 does them
 *             (V(new_state) with the old weights, the old W2 in the gradient); state = new_state; last_reward = reward
 *   refused:  no step, no update: state and weights unchanged
 *   rewards[t] = last_reward: a refused step repeats the last admitted step's reward, as the reference's list does; NaN
 *             until the first admission, where the reference appends nothing
 * An agent with gated[a] == 0 computes no look-ahead and takes every step: its rewards, weights, state, actor-update
 * count and status have the bits of sw_cacla_run_f64(train = 1); its violations are counted too.
 *   real          : the real swimmer (Gym model)
 *   gamma, alpha, noise, weights, state, rewards, status : as sw_cacla_run_f64
 *   gated         : [n_agent]  0: no gate
 *   sim           : [n_agent][3] (l_i, m_i, k) of each agent's simulator, read for gated agents only; the constants are
 *                   derived in the kernel by the function the host uses
 *   sim_thresh    : [n_agent], read for gated agents only;  real_thresh : [n_agent]
 *   cost_kind, cost_index : SW_COST_* as sw_safe_rollouts_f64
 *   last_reward   : in/out [n_agent]; set it to NaN before the first launch of a run
 *   admitted_rec  : NULL or [n_agent][n_iter], 1 / 0 per step
 *   counters      : in/out [n_agent][3], += admitted steps, violations, actor updates; zero them before a run
 *   first_refused : in/out [n_agent]; set it to -1 before a run: the kernel writes t_begin + t at the first refused
 *                   step t while it is still -1
 * A gated agent whose simulator breaks the parameter rule (SW_ERR_PARAM's) gets SW_STATUS_PARAM and every step refused;
 * the other agents are unaffected.  Everything an agent carries is in/out, so a run can be split into launches
 * (t_begin = the steps already run) and the split changes no bit.
 * Errors, before any HIP call: a NULL pointer other than admitted_rec / status SW_ERR_NULL; n_agent < 1, n_agent >
 * 2^31 - 1, n_iter < 0, t_begin < 0, t_begin + n_iter > 2^31 - 1, an unknown cost_kind or a cost_index outside 0..d-1
 * with SW_COST_ABS_OBS SW_ERR_SIZE; twin model SW_ERR_PARAM; n outside 2..8 SW_ERR_SEGMENTS.  n_iter = 0 writes
 * nothing. */
int sw_cacla_safe_run_f64(const sw_params *real, int64_t n_agent, int32_t n_iter, int64_t t_begin,
                          const double *gamma, const double *alpha, const double *noise,
                          const int32_t *gated, const double *sim, const double *sim_thresh,
                          const double *real_thresh, int32_t cost_kind, int32_t cost_index,
                          double *weights, double *state, double *last_reward, double *rewards,
                          int32_t *admitted_rec, int32_t *counters, int32_t *first_refused,
                          int32_t *status, void *stream);

/* ---- CACLA on the swimmer, every step gated on an ENSEMBLE of simulators: sw_cacla_safe_run_f64 with the look-ahead
 * in n_member simulators per agent (the CACLA side of sw_ars_gate_ensemble_f64: the members stand for the uncertainty
 * about (l_i, m_i, k), and a step is taken only where every one of them admits it) ----
 * sw_cacla_safe_ensemble_run_f64 runs n_iter steps for n_agent agents, one wave each, always training.  The members
 * ride in the lanes of the agent's wave -- lane L looks ahead in member L % n_member -- so an agent has at most 64 of
 * them: MORE THAN ONE WAVE'S WORTH OF MEMBERS IS NOT BUILT.  Step t of a gated agent:
 *   FA_act = actors(state); action = FA_act + noise[t]   (consumed whether or not the step is taken)
 *   c_e = cost(step(state, action) with member e's constants)     for every member e (n, h, direction are `real`'s)
 *   admitted = c_e <= sim_thresh[a] for EVERY e           (a NaN cost or threshold refuses)
 *   admitted / refused: as sw_cacla_safe_run_f64, and so are rewards, last_reward, counters, first_refused, t_begin and
 *             the status bits
 * With n_member = 1, or with n_member copies of one simulator, every output has the bits of sw_cacla_safe_run_f64 in
 * that simulator; an agent with gated[a] == 0 reads neither sims nor sim_thresh and has the bits of
 * sw_cacla_run_f64(train = 1).  The order of an agent's members changes nothing but the order of member_refusals.
 *   real, gamma, alpha, noise, gated, sim_thresh, real_thresh, cost_kind, cost_index, weights, state, last_reward,
 *   rewards, admitted_rec, counters, first_refused, status : as sw_cacla_safe_run_f64
 *   n_member      : 1..64, the same for every agent
 *   sims          : [n_agent][n_member][3] (l_i, m_i, k) of each member, read for gated agents only; the constants are
 *                   derived in the kernel by the function the host uses
 *   worst_rec     : NULL or [n_agent][n_iter]: the largest member cost of step t, admitted or refused; a NaN cost or a
 *                   member that breaks the parameter rule counts as +inf (NaN -> +inf per member first, then the
 *                   maximum: exact in any order).  On an admitted step worst_rec <= sim_thresh, on a refused one it is
 *                   larger (or the threshold is NaN).  NaN for an ungated agent
 *   member_refusals : NULL or in/out [n_agent][n_member], += the steps at which member e's own cost was not
 *                   <= sim_thresh, whatever the other members said (which member binds); zero it before a run.
 *                   Untouched for an ungated agent
 * A gated agent with a member that breaks the parameter rule (SW_ERR_PARAM's) gets SW_STATUS_PARAM and every step
 * refused (that member's constants are not used; its refusals count every step, worst_rec is +inf); the other agents
 * are unaffected.  A run can be split into launches as with sw_cacla_safe_run_f64, and the split changes no bit.
 * Errors, before any HIP call: those of sw_cacla_safe_run_f64 (worst_rec and member_refusals may be NULL as well), and
 * n_member < 1 or n_member > 64 SW_ERR_SIZE.  n_iter = 0 writes nothing. */
int sw_cacla_safe_ensemble_run_f64(const sw_params *real, int64_t n_agent, int32_t n_member, int32_t n_iter,
                                   int64_t t_begin, const double *gamma, const double *alpha, const double *noise,
                                   const int32_t *gated, const double *sims, const double *sim_thresh,
                                   const double *real_thresh, int32_t cost_kind, int32_t cost_index, double *weights,
                                   double *state, double *last_reward, double *rewards, int32_t *admitted_rec,
                                   double *worst_rec, int32_t *member_refusals, int32_t *counters,
                                   int32_t *first_refused, int32_t *status, void *stream);

/* ---- CACLA on LQR, with and without safe exploration (cacla/cacla_agent.py:202-297, cacla/cacla_safe_agent.py,
 * envs/gym_lqr/lqr_env.py): whole runs of many independent agents in ONE launch, one agent per lane ----
 * sw_lqr_cacla_run_f64 runs n_iter steps of the reference's `run` loops for n_agent agents with state dimension ns
 * (1..SW_LQR_MAX_STATE) and action dimension na (1..SW_LQR_MAX_ACTION).  One step (clip = reset_inbound as coded,
 * lqr_env.py:80-93: bound M == 0 is no bound, otherwise |x| > M -> |x| / x * M):
 *   fa = F s;  u = fa + noise[t]
 *   safe: thr = the agent's fixed one (SW_LQR_THRESHOLD_FIXED), or l - eps_Lc (dA ||s||_2 + dB ||u||_2) (.._STEP; u
 *         unclipped);  s_sim = clip_s(A_sim s + B_sim clip_a(u) + C_sim);  admitted = cost(s_sim) <= thr
 *   admitted (always when safe == 0):
 *         a = clip_a(u);  s' = clip_s(A s + B a + C);  r = -(s'^T Q s' + a^T R a)
 *         safe and not cost(s') <= l: violations += 1        (the reference prints a line)
 *         td = r + gamma sum_j V_j s'_j^2 - sum_j V_j s_j^2;  V_j += alpha td s_j^2
 *         td > 0: F_ij += alpha (u_i - fa_i) s_j  (u unclipped, fa from before);  actor_updates += 1
 *         last = (s, a, r);  s = s';  admitted += 1
 *   refused: nothing changes
 *   record of step t = last, flag SW_LQR_ADMITTED / SW_LQR_REFUSED (last repeats the last admitted step, as the
 *         reference's lists do) / SW_LQR_NOTHING_YET (refused and nothing admitted so far in the run: no entry)
 * Arithmetic is not trapped: NaN and inf propagate, a NaN cost refuses, a NaN td updates no actor.
 * EVERY array is agent-minor ([..][n_agent]): a wave's 64 agents read and write one contiguous run, and the noise and
 * the records are step-major, so a step's traffic is a handful of such runs.
 *   params   : [SW_LQR_PARAM_DOUBLES(ns, na)][n_agent]: the real model, the simulator's model (each
 *              SW_LQR_MODEL_DOUBLES: A [ns][ns] row-major | B [ns][na] | C [ns] | max_s | max_a; C = 0 and bound 0 for
 *              what an environment does not have), Q [ns][ns], R [na][na], gamma, alpha, l, eps_Lc = epsilon * L_c,
 *              dA = op_norm_der_A, dB = op_norm_der_B, the fixed simulator threshold.  safe == 0 reads the real
 *              model, Q, R, gamma and alpha only
 *   noise    : [n_iter][na][n_agent], added to F s: the caller's N(0, sigma) draws
 *   F        : in/out [na][ns][n_agent];  V, state: in/out [ns][n_agent]
 *   last     : in/out [ns + na + 1][n_agent]: the last admitted step's (s, a, r); meaningful once admitted > 0
 *   counters : in/out int32 [3][n_agent]: admitted, violations, actor_updates; zero them before a run
 *   status   : in/out int32 [n_agent], |= SW_STATUS_NONFINITE when F, V or the state is not finite after the call
 *   rec_state [n_iter][ns][n_agent] (the state BEFORE the step), rec_action [n_iter][na][n_agent] (clipped),
 *   rec_reward [n_iter][n_agent], rec_admitted uint8 [n_iter][n_agent]: each NULL or written at every step
 * Everything an agent carries is in/out, so a run can be split into launches and the split changes no bit.
 * cost: SW_LQR_COST_INF max_j |x_j|, SW_LQR_COST_2 sqrt(sum x_j^2), SW_LQR_COST_1 sum |x_j|.
 * Errors, before any HIP call: a NULL pointer other than a record SW_ERR_NULL; n_agent < 1, n_agent > 2^31 - 1,
 * n_iter < 0, ns or na out of range SW_ERR_SIZE; safe not 0 / 1, unknown threshold or cost SW_ERR_PARAM.
 * n_iter = 0 writes nothing. */
#define SW_LQR_MAX_STATE 4
#define SW_LQR_MAX_ACTION 2
#define SW_LQR_MODEL_DOUBLES(ns, na) ((ns) * (ns) + (ns) * (na) + (ns) + 2)
#define SW_LQR_PARAM_DOUBLES(ns, na) (2 * SW_LQR_MODEL_DOUBLES(ns, na) + (ns) * (ns) + (na) * (na) + 7)
#define SW_LQR_THRESHOLD_STEP 0  /* CACLA_LQR_SE_agent */
#define SW_LQR_THRESHOLD_FIXED 1 /* CACLA_LQR_SE_fix, CACLA_Bounded_LQR_SE_agent, CACLA_AffineQR_SE_agent */
#define SW_LQR_COST_INF 0
#define SW_LQR_COST_2 1
#define SW_LQR_COST_1 2
#define SW_LQR_REFUSED 0
#define SW_LQR_ADMITTED 1
#define SW_LQR_NOTHING_YET 2
int sw_lqr_cacla_run_f64(int32_t ns, int32_t na, int64_t n_agent, int32_t n_iter, int32_t safe, int32_t threshold,
                         int32_t cost, const double *params, const double *noise, double *F, double *V, double *state,
                         double *last, int32_t *counters, int32_t *status, double *rec_state, double *rec_action,
                         double *rec_reward, uint8_t *rec_admitted, void *stream);

/* ---- The RL-Glue ARS experiment on the native swimmer (rlglue/agent/SwimmerAgent.py:61-130, :167-239 driven by
 * rlglue/experiment/SwimmerExperiment.cpp:65-84 on rlglue/environment/SwimmerEnvironment.cpp): whole training runs of
 * many independent agents in ONE launch, one agent per lane ----
 * sw_rlglue_ars_run_f64 runs n_iter iterations for n_agent agents with N directions, b of them used, segments of H
 * environment steps.  d = 2n + 2, m = n - 1, s0 = the start state (every component 0.001, SwimmerEnvironment.cpp:41),
 * clip = the agent's `if a > max_u: a = max_u elif a < -max_u: a = -max_u` (SwimmerAgent.py:192-196; a NaN passes):
 *   pol(j) = P + nu delta[j / 2] (j even) | P - nu delta[j / 2] (j odd)        (:210-212; delta = np.random.rand)
 *   before the first iteration: stale = clip(pol(0) s0), total = 0              (agent_start, :61-77)
 *   segment(W, stale): s = s0 ("load state"), a = stale; for t = 0 .. H - 1: s, r = twin_step(s, a);
 *         t == 0: first = r, a = clip(W s0)     (the agent answers the first step with the INITIAL observation, :96)
 *         else:   rest += r, a = clip(W s);      -> first, rest, a (= the next segment's stale action)
 *   iteration: for j = 0 .. 2N - 1: first, rest, stale = segment(pol(j), stale);
 *                  rew[(j - 1) mod 2N] = total + first; total = rest            (credited one segment late, :88-93)
 *              sigma = sample standard deviation of rew[0 .. 2b)                 (:227-231; index order, no sort)
 *              P += alpha (sum_{i < b} (rew[2i] - rew[2i + 1]) delta[i]) / (b sigma)                      (:233-239)
 *              first, rest, stale = segment(P, stale); total = rest; report rest (frozen evaluation, :100-104)
 * So rew[2N - 1] is the evaluation's return before it plus segment 0's first reward, segment 2N - 1's return reaches
 * no update, and directions b .. N - 1 are rolled out but not used.  Arithmetic is not trapped: NaN and inf propagate
 * (the reference's statistics.stdev raises on a NaN return; here the agent's status gets SW_STATUS_NONFINITE).
 * EVERY array is agent-minor ([..][n_agent]):
 *   alpha, nu     : [n_agent]
 *   deltas        : [n_iter][N][m][d][n_agent]: the caller's draws for the iterations of THIS call
 *   policy        : in/out [m][d][n_agent]
 *   carry         : in/out [m + 1][n_agent]: the stale action, then total; iter_begin == 0 ignores it on input (the
 *                   kernel forms clip(pol(0) s0) itself)
 *   eval_returns  : [n_iter][n_agent]: the line SwimmerExperiment.cpp:83 writes
 *   train_returns : [n_iter][2N][n_agent]: rew as the update saw it (required: the lane reads its own values back)
 *   status        : in/out int32 [n_agent], |= SW_STATUS_SINGULAR / SW_STATUS_NONFINITE (a state, a return or a
 *                   policy entry was not finite) / SW_STATUS_RANGE (values are NOT replaced by NaN here)
 * Everything an agent carries is in/out, so a run can be split into launches and the split changes no bit.  max_u is
 * an argument, not a field of sw_params; +inf means no clip.  p must carry SW_FLAG_MODEL_TWIN.
 * Errors, before any HIP call: NULL pointer SW_ERR_NULL; n_agent < 1, n_agent > 2^31 - 1, n_iter < 0, iter_begin < 0,
 * N < 1, b < 1, b > N (the reference raises IndexError) or H < 1 SW_ERR_SIZE; n outside 2..8 SW_ERR_SEGMENTS; model
 * bit clear, or max_u NaN or negative SW_ERR_PARAM.  n_iter = 0 writes nothing. */
int sw_rlglue_ars_run_f64(const sw_params *p, double max_u, int64_t n_agent, int64_t iter_begin, int32_t n_iter,
                          int32_t N, int32_t b, int32_t H, const double *alpha, const double *nu,
                          const double *deltas, double *policy, double *carry, double *eval_returns,
                          double *train_returns, int32_t *status, void *stream);

/* The same update reading an all-gathered buffer in place (no repacking between the
 * collective and the update):  gathered = `world` segments of
 * seg_len = 2*chunk + rows_chunk*2d doubles, segment r =
 * [2*chunk returns of directions r*chunk .. | rows_chunk moment rows]  (zero padded).
 * world = 1 is a single rank's own segment. */
int sw_ars_update_gathered_f64(const sw_params *p, int64_t n_dir, const double *gathered,
                               int32_t world, int64_t chunk, int64_t rows_chunk,
                               const double *deltas, double *policy, double alpha, double b,
                               int64_t top_b, double *running, int64_t n_new_states,
                               double *mean, double *inv_std, double *sigma_out, void *stream);

/* Full first and second moments of recorded trajectories (for the `covariance` attribute):
 * acc[0] += count, acc[1..d] += sum(s - c), acc[1+d + f*d + g] += sum((s-c)_f (s-c)_g),
 * over traj [H][d][n_roll].  HBM-bound: reads the trajectory buffer exactly once.
 * acc holds sw_cov_acc_doubles(p, n_roll, H) doubles: the 1 + d + d*d sums, then the pass's
 * scratch (a ticket counter and the tiles' partial sums, laid out [entry][tile]); the caller zeroes
 * ALL of it before the first call and leaves the scratch part alone afterwards.  No floating-point
 * atomics: the tile that finishes last merges the partial sums in an order that depends on the
 * number of tiles only, so the same call on the same data gives the same bits.  Passes over one acc
 * must be stream-ordered (one at a time). */
int64_t sw_cov_acc_doubles(const sw_params *p, int64_t n_roll, int32_t H);
int sw_traj_moments_f64(const sw_params *p, int64_t n_roll, int32_t H, const double *traj,
                        double *acc, void *stream);


/* ---- one swimmer, one step per call: the batch-1 drop-in surfaces -------------------------
 * SwimmerEnv.step / next_observation (remy_swimmer_env.py:41-56, :69-93) and the native twin's
 * env_step (rlglue/environment/SwimmerEnvironment.cpp:53-68) hand over ONE state and ONE action
 * and need the next state before they return.  A handle owns a small pinned, device-mapped
 * I/O block and a stream of its own: the caller writes state and action into the block,
 * sw_env1_step launches ONE kernel that reads them over the bus, writes next state, reward and
 * status back into the block and then a sequence number the host spins on -- one launch and
 * one host wait per step; no allocation, no memcpy call, no stream synchronisation.
 * Offsets into the block, in doubles (sized for SW_MAX_SEGMENTS): */
#define SW_ENV1_STATE 0    /* in : [d]  observation order [Gdx, Gdy, th1, thd1, ...] */
#define SW_ENV1_ACTION 18  /* in : [m] */
#define SW_ENV1_NEXT 32    /* out: [d]  (sw_env1_step) */
#define SW_ENV1_REWARD 50  /* out: [1]  (sw_env1_step) */
#define SW_ENV1_GDD 52     /* out: [2]  (sw_env1_accel) */
#define SW_ENV1_TDD 54     /* out: [n]  (sw_env1_accel) */
#define SW_ENV1_DOUBLES 64
typedef struct sw_env1 sw_env1;
int sw_env1_create(sw_env1 **out);
void sw_env1_destroy(sw_env1 *e);
/* A handle is used by one thread at a time (it owns one I/O block and one sequence counter) and
 * belongs to the device that was current when it was created: sw_env1_step / sw_env1_accel launch on that
 * device whatever the caller's current device is, and leave the caller's current device unchanged.
 * HOST pointer to the handle's I/O block (SW_ENV1_DOUBLES doubles), valid until destroy. */
double *sw_env1_io(sw_env1 *e);
/* One physics step of the swimmer in the block (model chosen by p->flags); BLOCKING: the
 * outputs are in the block when it returns.  *status (host, may be NULL) receives SW_STATUS_*. */
int sw_env1_step(sw_env1 *e, const sw_params *p, int32_t *status);
/* compute_accelerations of the state / action in the block (remy_swimmer_env.py:95-114). */
int sw_env1_accel(sw_env1 *e, const sw_params *p);

/* ---- the exchange step of the sharded ARS iteration, straight into RCCL -----------------
 * One all-gather of every rank's packed result segment per iteration replaces the serial loop
 * over directions (ars/ars_agent.py:160 "TODO ... PARALLEL"); see sw_ars_update_gathered_f64 for
 * the layout.  These entry points issue it from native code ON THE CALLER'S STREAM (the critical
 * stream rollouts -> all-gather -> update), without torch.distributed in between.  RCCL is
 * resolved at run time (dlopen by soname: the copy a torch process has loaded already), so the
 * library has no link-time dependency on it; sw_comm_available() says whether it was found.
 * Rank 0 draws the id, the caller distributes its SW_COMM_ID_BYTES bytes by whatever means it has
 * (torch.distributed broadcast, MPI, a file), every rank creates its communicator (collective). */
#define SW_COMM_ID_BYTES 128
/* sw_comm_create is COLLECTIVE over the ranks and binds the communicator to the CURRENT device
 * (hipSetDevice first); one communicator per rank, one GPU per rank. */
typedef struct sw_comm sw_comm;
int sw_comm_available(void);
int sw_comm_unique_id(uint8_t *id /* host, SW_COMM_ID_BYTES */);
int sw_comm_create(sw_comm **out, const uint8_t *id, int32_t world, int32_t rank);
void sw_comm_destroy(sw_comm *c);
/* recv[r * count .. (r+1) * count) <- rank r's send[0 .. count)  (device pointers). */
int sw_comm_all_gather_f64(sw_comm *c, const double *send, double *recv, int64_t count, void *stream);
const char *sw_comm_last_error(sw_comm *c);

/* ---- measurement aid ---------------------------------------------------------------------
 * One wave issuing trips x 64 independent instructions of one class (mode 0: v_fma_f64,
 * mode 1: v_mov_b32); scratch64: 64 doubles.  bench.py times it with HIP events to calibrate the
 * ceiling of the latency-bound rollout kernels (one instruction per ~2 ns for a lone wave) on the
 * device it runs on.  Replaces nothing in the reference. */
int sw_issue_probe(int32_t mode, int32_t trips, double *scratch64, void *stream);
/* The same with `workgroups` x `waves_per_workgroup` (1..4) such waves at once: 256 x 4 puts one wave on
 * every SIMD of an MI355X, i.e. the intervals with the whole chip issuing (a chip full of f64 work sustains
 * a lower clock than a lone wave sees: bench.py prices the full-chip launches with these). */
int sw_issue_probe_grid(int32_t mode, int32_t trips, int32_t workgroups, int32_t waves_per_workgroup,
                        double *scratch64, void *stream);

/* ---- host helper: the reference's random stream ----------------------------------------
 * out[i] = 2*u_i - 1 with u_i the next doubles of NumPy's legacy MT19937 generator
 * (np.random.rand), continuing from the state (key[624], *pos) in the form
 * np.random.get_state() / set_state() use; the state is advanced in place.  Replaces the
 * N calls of 2*np.random.rand(m, d)-1 in ars/ars_agent.py:137-138 (same values, an order of
 * magnitude faster, so the host keeps ahead of the GPU at any rank count).  HOST pointers.
 * The vector width (baseline x86-64 / AVX2 / AVX-512) is chosen at run time from the CPU's features;
 * every width produces the same bits. */
int sw_mt19937_uniform_pm1(uint32_t *key, int32_t *pos, int64_t n, double *out);
/* Test hook: run the stream at a given width (0 baseline, 1 AVX2, 2 AVX-512; -1 = widest available, the
 * default); a width the CPU lacks falls back to the next one down.  Returns the width that will run. */
int sw_mt19937_force_isa(int level);

/* ---- ARS iteration pipeline (host-side enqueue logic in native code) ------------------
 * Replaces the serial body of ARSAgent.runOneIteration (ars/ars_agent.py:137-182) with a
 * schedule over a ring of SW_PIPELINE_SLOTS buffer sets.  A pipeline owns one extra HIP stream
 * (H2D copies of the deltas) and 64 bytes of pinned host memory (a progress flag); it owns no
 * device memory: every buffer is passed per call, one set per `slot`.  The slot of a call is
 * sw_ars_pipeline_next_slot() = (number of sw_ars_iteration_rollouts_f64 calls so far) mod
 * SW_PIPELINE_SLOTS -- the pipeline's own count, so that a caller's iteration counter (reset by
 * a checkpoint load, say) can never shift the ring; a call with another slot is refused with
 * SW_ERR_SIZE.  Every rank calls once per iteration, also with an empty shard (n_dir = 0: nothing
 * but the progress flag is launched).  Use the pipeline with ONE stream.  The caller's stream carries kernels
 * only -- no cross-stream waits, no event records: every rollout launch stores its index to the
 * progress flag when it starts, and the host paces buffer reuse on that.
 *
 *   sw_ars_iteration_rollouts_f64   copy stream: deltas_host (pinned) -> deltas_dev
 *                                   caller's stream: ONE launch = the 2*n_dir rollouts of this
 *                                   rank's shard + (extra workgroups) the covariance pass
 *                                   sw_traj_moments_f64 over the PREVIOUS call's traj -> its
 *                                   cov_acc; this call's traj is owed a pass (if cov_acc given;
 *                                   cov_acc: sw_cov_acc_doubles(p, 2*n_dir, H) doubles, zeroed)
 *   ... caller all-gathers its segment [returns | moment rows] between ranks ...
 *   sw_ars_iteration_update_f64     caller's stream: sw_ars_update_gathered_f64 on the gathered
 *                                   buffer
 *
 * Before refilling deltas_host of a slot the host calls sw_ars_pipeline_host_slot_wait;
 * before reading cov_acc it calls sw_ars_pipeline_sync_cov (runs the pass still owed and
 * synchronises the stream). */
#define SW_PIPELINE_SLOTS 4
typedef struct sw_ars_pipeline sw_ars_pipeline;

int sw_ars_pipeline_create(sw_ars_pipeline **out);
void sw_ars_pipeline_destroy(sw_ars_pipeline *pl);
int sw_ars_pipeline_slots(void);
int sw_ars_pipeline_next_slot(sw_ars_pipeline *pl);
int sw_ars_pipeline_host_slot_wait(sw_ars_pipeline *pl, int slot);
int sw_ars_pipeline_sync_cov(sw_ars_pipeline *pl);
/* enable = k > 0: record HIP events around every k-th rollout launch on its stream (resets the
 * log; each timed launch costs ~10 us of pipeline bubbles, so sample sparsely); 0: off */
int sw_ars_pipeline_timing(sw_ars_pipeline *pl, int enable);
int sw_ars_pipeline_rollout_ms(sw_ars_pipeline *pl, double *mean_ms, int64_t *launches);

int sw_ars_iteration_rollouts_f64(sw_ars_pipeline *pl, int slot, const sw_params *p,
                                  int64_t n_dir_total, int64_t dir_begin, int64_t n_dir,
                                  int32_t H, const double *deltas_host /* pinned host */,
                                  double *deltas_dev, const double *policy, double nu,
                                  const double *mean, const double *inv_std, double *returns,
                                  double *traj, double *moments, double *cov_acc,
                                  int32_t *status, void *stream);

int sw_ars_iteration_update_f64(sw_ars_pipeline *pl, int slot, const sw_params *p,
                                int64_t n_dir, const double *gathered, int32_t world,
                                int64_t chunk, int64_t rows_chunk, const double *deltas_dev,
                                double *policy, double alpha, double b, int64_t top_b,
                                double *running, int64_t n_new_states, double *mean,
                                double *inv_std, double *sigma_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWIMMER_HIP_H */
