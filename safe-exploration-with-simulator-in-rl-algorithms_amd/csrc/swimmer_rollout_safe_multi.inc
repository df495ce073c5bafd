// Per-agent view of sw_safe_ars_rollouts_multi_f64: included INSIDE a safe_ars_multi_*_kernel's braces, in FRONT of its
// form's safe body (swimmer_rollout_safe_*.inc with SW_SAFE_MULTI 1), with SW_MULTI_N = the segment count and
// SW_MULTI_SLOTS = the rollouts a workgroup of the form has lanes for.  The grid is (workgroups of one agent, n_agent),
// as in swimmer_rollout_multi.inc: workgroup (x, a) is workgroup x of agent a, n_roll stays the rollouts PER AGENT, and
// the names the body reads become agent a's: its policy and deltas, its slices of the outputs, whether it is gated at
// all, its real threshold and -- for a gated agent -- its simulator's constants (derived from all.sim with
// sw::consts_of: the host's bits) and simulator threshold.  An ungated agent reads neither all.sim nor
// all.sim_thresh; Cs is then the real swimmer's and never used.
// A gated agent whose simulator breaks the parameter rule: SW_STATUS_PARAM, NaN returns, cost trace and maximum,
// first_refused 0, no violations -- the convention of sw_ars_gate_multi_f64.
    constexpr int kAgentD = 2 * (SW_MULTI_N) + 2, kAgentM = (SW_MULTI_N) - 1;
    const int64_t agent = blockIdx.y;
    const bool gated = __builtin_amdgcn_readfirstlane(all.gated[agent]) != 0;
    const double *__restrict__ const policies = all.policy + agent * (kAgentM * kAgentD);
    const double *__restrict__ const deltas = all.deltas + agent * (n_roll >> 1) * (kAgentM * kAgentD);
    double *__restrict__ const returns = all.returns + agent * n_roll;
    double *__restrict__ const cost_max = all.cost_max ? all.cost_max + agent * n_roll : nullptr;
    int32_t *__restrict__ const first_refused = all.first_refused ? all.first_refused + agent * n_roll : nullptr;
    int32_t *__restrict__ const violations = all.violations ? all.violations + agent * n_roll : nullptr;
    int32_t *__restrict__ const status = all.status ? all.status + agent * n_roll : nullptr;
    double *const traj = nullptr;
    const double real_thresh = uniform_f64(all.real_thresh[agent]);
    double sim_thresh = 0.0;
    sw::Consts Cs = Cr;
    if (gated) {   // uniform
        const double sim_l = all.sim[agent * 3], sim_m = all.sim[agent * 3 + 1], sim_k = all.sim[agent * 3 + 2];
        if (!sim_params_ok(sim_l, sim_m, sim_k)) {
            const int64_t r_bad = (int64_t)blockIdx.x * (SW_MULTI_SLOTS) + threadIdx.x;
            if ((int)threadIdx.x < (SW_MULTI_SLOTS) && r_bad < n_roll) {
                returns[r_bad] = __builtin_nan("");
                if (status) status[r_bad] = SW_STATUS_PARAM;
                if (first_refused) first_refused[r_bad] = 0;
                if (violations) violations[r_bad] = 0;
                if (cost_max) cost_max[r_bad] = __builtin_nan("");
                if (all.cost_trace)
                    for (int32_t t = 0; t < H; ++t)
                        all.cost_trace[((int64_t)t * gridDim.y + agent) * n_roll + r_bad] = __builtin_nan("");
            }
            return;
        }
        Cs = uniform_consts(sw::consts_of(SW_MULTI_N, sim_l, sim_m, sim_k, Cr.h, Cr.dirx, Cr.diry));
        sim_thresh = uniform_f64(all.sim_thresh[agent]);
    }
    const sw::Consts Creal = Cr, Csim = Cs;   // the lane body's names
    const double tq_ratio = Cs.c12 / Cr.c12;  // the mirror-quad body's: IEEE division, the host's bits
