// Body of safe_rollout_kernel (csrc/swimmer_rollout_lane.hip), shared with its multi-agent ARS form
// (sw_safe_ars_rollouts_multi_f64, csrc/swimmer_rollout_safe_multi.hip): included INSIDE the kernels' braces with
// SW_SAFE_MULTI 0 (the safe-rollout kernel, the machine code it had) or 1 (behind swimmer_rollout_safe_multi.inc, the
// per-agent view: the policy is P + / - nu delta, `gated` -- workgroup-uniform -- decides whether the rollout looks
// ahead at all, and the cost of the state the reference appends at step t goes to cost_trace / cost_max instead of the
// state to a trajectory).
// SW_SAFE_ENSEMBLE 1 (with SW_SAFE_MULTI 1; sw_safe_ars_rollouts_ensemble_f64, csrc/swimmer_safe_ars_ensemble.hip): a
// rollout owns a GROUP of lanes, each with the constants of one member of the agent's simulator ensemble in Csim.  The
// kernel has placed the lane already -- r, and `owner`, the one lane of the group that stores -- and the gate is a wave
// ballot over the group: `member_bits` (kernel) cuts this group's members out of it.  A group leaves the loop whole.
    constexpr int D = 2 * N + 2, M = N - 1;
#if !SW_SAFE_ENSEMBLE
    const int64_t r = (int64_t)blockIdx.x * kRollBlock + threadIdx.x;
    if (r >= n_roll) return;
    constexpr bool owner = true;
#endif
    double W[M][D];
#if SW_SAFE_MULTI
    {   // P + / - nu delta with NumPy's rounding (rollout_kernel's prologue, swimmer_rollout_lane.inc)
        const double sgn = (r & 1) ? -1.0 : 1.0;
        const double *dl = deltas + (r >> 1) * (M * D);
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) W[i][j] = __dadd_rn(policies[i * D + j], sgn * __dmul_rn(nu, dl[i * D + j]));
    }
    double cnow = 0.0, cmax = 0.0;                    // cost of the current state; costs are >= 0 or NaN
    double *const trace = (owner && all.cost_trace) ? all.cost_trace + agent * n_roll + r : nullptr;
    const int64_t trace_step = (int64_t)gridDim.y * n_roll;   // cost_trace [H][n_agent][n_roll], grid.y = n_agent
    auto nan_max = [](double a, double b) { return __builtin_isunordered(a, b) ? __builtin_nan("") : fmax(a, b); };
#else
    const double *pl = policies + r * (M * D);
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) W[i][j] = pl[i * D + j];
#endif
    double gdx = 0.0, gdy = 0.0, th[N], thd[N];      // real_env.reset() (:133)
#pragma unroll
    for (int i = 0; i < N; ++i) {
        th[i] = kHalfPi;
        thd[i] = 0.0;
    }
    auto record = [&](int32_t t) {
        double *tp = traj + (int64_t)t * D * n_roll + r;
        tp[0] = gdx;
        tp[n_roll] = gdy;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            tp[(int64_t)(2 + 2 * i) * n_roll] = th[i];
            tp[(int64_t)(3 + 2 * i) * n_roll] = thd[i];
        }
    };
    double total = 0.0, thmax = 0.0;
    bool ok = true;
    int32_t refused_at = H, over = 0;
    for (int32_t t = 0; t < H; ++t) {
        thmax = sw::track_angle_range<N>(thmax, th);
        double sm[D];
        sm[0] = gdx;
        sm[1] = gdy;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            sm[2 + 2 * i] = th[i];
            sm[3 + 2 * i] = thd[i];
        }
        double u[M];                                  // ac = policy @ obs (:139)
#pragma unroll
        for (int i = 0; i < M; ++i) {
#if SW_SAFE_MULTI
            // a Basic_ARS rollout is rollout_kernel's: its first partial sum starts from the (zero) V1 bias, which
            // differs from the bare product in the sign of a zero only
            double a0 = gated ? W[i][0] * sm[0] : __builtin_fma(W[i][0], sm[0], 0.0), a1 = W[i][1] * sm[1];
#else
            double a0 = W[i][0] * sm[0], a1 = W[i][1] * sm[1];
#endif
#pragma unroll
            for (int j = 2; j < D; j += 2) {
                a0 = __builtin_fma(W[i][j], sm[j], a0);
                a1 = __builtin_fma(W[i][j + 1], sm[j + 1], a1);
            }
            u[i] = a0 + a1;
        }
#if SW_SAFE_MULTI
        if (gated) {   // uniform: a Basic_ARS rollout takes every step (safe_ars/ars.py:20-31)
#endif
        // the simulator's look-ahead from the real state (:120-121)
        double sgx = gdx, sgy = gdy, sth[N], sthd[N], srew;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            sth[i] = th[i];
            sthd[i] = thd[i];
        }
        (void)sw::euler_step<N>(Csim, sgx, sgy, sth, sthd, u, srew);
#if SW_SAFE_ENSEMBLE
        // every lane its member's verdict; the group's through one ballot: all of its lanes see the same bits
        const double c_mem = safe_cost<N>(cost_kind, cost_index, sgx, sgy, sth, sthd);
        const uint64_t out = member_bits(__builtin_amdgcn_ballot_w64(!(c_mem <= sim_thresh)));   // NaN refuses
        if (out) {
            refused_at = t;
            refusing = out;
            break;
        }
        if (want_worst) worst = fmax(worst, c_mem);   // uniform; an admitted cost is no NaN
#else
        if (!(safe_cost<N>(cost_kind, cost_index, sgx, sgy, sth, sthd) <= sim_thresh)) {   // :122, NaN refuses
            refused_at = t;
            break;
        }
#endif
#if SW_SAFE_MULTI
        }
#endif
        double rew;
        ok = sw::euler_step<N>(Creal, gdx, gdy, th, thd, u, rew) && ok;                     // :142
        total += rew;
#if SW_SAFE_MULTI
        cnow = safe_cost<N>(cost_kind, cost_index, gdx, gdy, th, thd);
        over += (cnow > real_thresh) ? 1 : 0;                                                     // :143-144
        cmax = nan_max(cmax, cnow);
        if (trace) trace[t * trace_step] = cnow;
#else
        over += (safe_cost<N>(cost_kind, cost_index, gdx, gdy, th, thd) > real_thresh) ? 1 : 0;   // :143-144
        if (traj) record(t);
#endif
    }
#if SW_SAFE_MULTI
    if (refused_at < H) {                                        // :151: the unchanged state's cost, step after step
        if (refused_at == 0) cnow = safe_cost<N>(cost_kind, cost_index, gdx, gdy, th, thd);   // the reset state's
        cmax = nan_max(cmax, cnow);
        if (trace)
            for (int32_t t = refused_at; t < H; ++t) trace[t * trace_step] = cnow;
    }
    if (owner && cost_max) cost_max[r] = cmax;
#else
    if (traj)
        for (int32_t t = refused_at; t < H; ++t) record(t);      // :151: the unchanged state, step after step
#endif
    bool fin = isfinite(gdx) && isfinite(gdy);
#pragma unroll
    for (int i = 0; i < N; ++i) fin = fin && isfinite(th[i]) && isfinite(thd[i]);
    const bool in_range = thmax < sw::kAngleLimit;
    if (owner) {
        returns[r] = in_range ? total : __builtin_nan("");
        if (first_refused) first_refused[r] = refused_at;
        if (violations) violations[r] = over;
        if (status)
            status[r] =
                (ok ? 0 : SW_STATUS_SINGULAR) | (fin ? 0 : SW_STATUS_NONFINITE) | (in_range ? 0 : SW_STATUS_RANGE);
    }
