// Per-agent view of a multi-agent ARS launch (sw_ars_rollouts_multi_f64): included INSIDE a multi kernel's braces, in
// FRONT of its form's body (swimmer_rollout_*.inc), with SW_MULTI_N = the segment count.  The launch's grid is
// (workgroups of one agent, n_agent): workgroup (x, a) is workgroup x of agent a's own single-agent launch.  The names
// the body reads -- policies, deltas, mean, inv_std, returns, moments, status -- become that agent's slices of the
// agent-major arrays in `all` (sw_launch::MultiArgs), n_roll stays the rollouts PER AGENT, and the body then indexes,
// pads (surplus slots recompute the agent's last rollout and store nothing) and reduces its moment rows exactly as
// in a single-agent launch: workgroup-uniform base pointers, no moment row with two agents' states.
//
// Two more views for the safe batch (`all` is a sw_launch::SafeMultiArgs there):
//   SW_MULTI_COUNTED 1 (sw_ars_rollouts_multi_counted_f64): the kernel's argument is n_roll_max, which sets the
//     strides; n_roll = 2 count[agent] is read here.  A workgroup behind the agent's last rollout -- every workgroup
//     of an agent with count 0 -- returns at once: the test is workgroup-uniform and sits in front of every barrier.
//     SW_MULTI_SLOTS = the rollouts a workgroup of the form has lanes for.
//   SW_MULTI_GATE 1 (sw_ars_gate_multi_f64): the kernel's argument is `base` (n, h, direction); C comes from the
//     agent's (l_i, m_i, k) in all.sim through sw::consts_of -- the host's bits -- and gate_thr / admit are the
//     agent's.  A parameter set that breaks the parameter rule: SW_STATUS_PARAM, NaN returns, nothing admitted.
// One more for the ensemble gate (`all` is a sw_launch::EnsembleArgs there):
//   SW_MULTI_ENSEMBLE 1, with SW_MULTI_GATE 1 (sw_ars_gate_ensemble_f64): the grid is (workgroups of one agent,
//     n_agent * n_sim) and blockIdx.y = agent * n_sim + member.  What a rollout READS -- policy, deltas, mean, inv_std,
//     the threshold -- is the agent's, shared by its members and never replicated in memory; the simulator and what
//     the rollout WRITES -- returns, status, admit -- are the member's: SW_MULTI_OUT names whose slice an output is.
    constexpr int kAgentD = 2 * (SW_MULTI_N) + 2, kAgentM = (SW_MULTI_N) - 1;
#if SW_MULTI_ENSEMBLE
    const int64_t member = blockIdx.y;
    const int64_t agent = (uint32_t)blockIdx.y / (uint32_t)all.n_sim;
#define SW_MULTI_OUT member
#else
    const int64_t agent = blockIdx.y;
#define SW_MULTI_OUT agent
#endif
#if SW_MULTI_COUNTED
    const int32_t agent_dirs = __builtin_amdgcn_readfirstlane(all.count[agent]);
    const int64_t n_roll = 2 * (int64_t)(agent_dirs < 0 ? 0 : (agent_dirs > (n_roll_max >> 1) ? (n_roll_max >> 1) : agent_dirs));
    if ((int64_t)blockIdx.x * (SW_MULTI_SLOTS) >= n_roll) return;
#define SW_MULTI_STRIDE n_roll_max
#else
#define SW_MULTI_STRIDE n_roll
#endif
    const double *__restrict__ const policies = all.policy + agent * (kAgentM * kAgentD);
    const double *__restrict__ const deltas = all.deltas + agent * (SW_MULTI_STRIDE >> 1) * (kAgentM * kAgentD);
    const double *__restrict__ const mean = all.mean ? all.mean + agent * kAgentD : nullptr;
    const double *__restrict__ const inv_std = all.inv_std ? all.inv_std + agent * kAgentD : nullptr;
    double *__restrict__ const returns = all.returns + SW_MULTI_OUT * SW_MULTI_STRIDE;
#if SW_MULTI_GATE
    double *const moments = nullptr;
#else
    double *__restrict__ const moments =
        all.moments ? all.moments + agent * ((SW_MULTI_STRIDE + kMomGroup - 1) / kMomGroup) * (2 * kAgentD) : nullptr;
#endif
    int32_t *__restrict__ const status = all.status ? all.status + SW_MULTI_OUT * SW_MULTI_STRIDE : nullptr;
#undef SW_MULTI_STRIDE
    constexpr int64_t dir_begin = 0;
    const double *const state0 = nullptr;
    double *const traj = nullptr;
    double *const final_state = nullptr;
#if SW_MULTI_GATE
    int32_t *__restrict__ const admit = all.admit + SW_MULTI_OUT * (n_roll >> 1);
    const double gate_thr = uniform_f64(all.sim_thresh[agent]);
    const double sim_l = all.sim[SW_MULTI_OUT * 3], sim_m = all.sim[SW_MULTI_OUT * 3 + 1],
                 sim_k = all.sim[SW_MULTI_OUT * 3 + 2];
    if (!sim_params_ok(sim_l, sim_m, sim_k)) {   // uniform; in front of every barrier
        const int64_t r_bad = (int64_t)blockIdx.x * (SW_MULTI_SLOTS) + threadIdx.x;
        if ((int)threadIdx.x < (SW_MULTI_SLOTS) && r_bad < n_roll) {
            returns[r_bad] = __builtin_nan("");
            if (status) status[r_bad] = SW_STATUS_PARAM;
            if ((r_bad & 1) == 0) admit[r_bad >> 1] = 0;
        }
        return;
    }
    const sw::Consts C = uniform_consts(sw::consts_of(SW_MULTI_N, sim_l, sim_m, sim_k, base.h, base.dirx, base.diry));
#endif
#undef SW_MULTI_OUT
