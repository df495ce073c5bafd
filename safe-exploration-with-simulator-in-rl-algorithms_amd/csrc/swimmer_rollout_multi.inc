// Per-agent view of a multi-agent ARS launch (sw_ars_rollouts_multi_f64): included INSIDE a multi kernel's braces, in
// FRONT of its form's body (swimmer_rollout_*.inc), with SW_MULTI_N = the segment count.  The launch's grid is
// (workgroups of one agent, n_agent): workgroup (x, a) is workgroup x of agent a's own single-agent launch.  The names
// the body reads -- policies, deltas, mean, inv_std, returns, moments, status -- become that agent's slices of the
// agent-major arrays in `all` (sw_launch::MultiArgs), n_roll stays the rollouts PER AGENT, and the body then indexes,
// pads (surplus slots recompute the agent's last rollout and store nothing) and reduces its moment rows exactly as
// in a single-agent launch: workgroup-uniform base pointers, no moment row with two agents' states.
    constexpr int kAgentD = 2 * (SW_MULTI_N) + 2, kAgentM = (SW_MULTI_N) - 1;
    const int64_t agent = blockIdx.y;
    const double *__restrict__ const policies = all.policy + agent * (kAgentM * kAgentD);
    const double *__restrict__ const deltas = all.deltas + agent * (n_roll >> 1) * (kAgentM * kAgentD);
    const double *__restrict__ const mean = all.mean ? all.mean + agent * kAgentD : nullptr;
    const double *__restrict__ const inv_std = all.inv_std ? all.inv_std + agent * kAgentD : nullptr;
    double *__restrict__ const returns = all.returns + agent * n_roll;
    double *__restrict__ const moments =
        all.moments ? all.moments + agent * ((n_roll + kMomGroup - 1) / kMomGroup) * (2 * kAgentD) : nullptr;
    int32_t *__restrict__ const status = all.status ? all.status + agent * n_roll : nullptr;
    constexpr int64_t dir_begin = 0;
    const double *const state0 = nullptr;
    double *const traj = nullptr;
    double *const final_state = nullptr;
