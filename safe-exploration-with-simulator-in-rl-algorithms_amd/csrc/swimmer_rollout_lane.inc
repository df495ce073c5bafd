// Body of rollout_kernel (csrc/swimmer_rollout_lane.hip), shared with its sw_ars_gate_f64 form and its multi-agent form
// (sw_ars_rollouts_multi_f64): included INSIDE the kernels' braces with SW_GATE_BODY 0 (the rollout kernel, token for
// token what it was; the multi-agent kernel behind swimmer_rollout_multi.inc) or 1 (the gate).
    constexpr int D = 2 * N + 2, M = N - 1;
    const int64_t r = (int64_t)blockIdx.x * kRollBlock + threadIdx.x;
    const bool active = r < n_roll;
    const bool v2 = (mean != nullptr);

    double m1[D], m2[D];  // V2 moment sums of (s - c), c = reset state
#pragma unroll
    for (int j = 0; j < D; ++j) m1[j] = m2[j] = 0.0;

    if (active) {
        // ---- policy into registers ----
        double W[M][D];
        if (ARS) {
            const int64_t dir = dir_begin + (r >> 1);
            const double sgn = (r & 1) ? -1.0 : 1.0;
            const double *dl = deltas + dir * (M * D);
#pragma unroll
            for (int i = 0; i < M; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const double t = __dmul_rn(nu, dl[i * D + j]);
                    W[i][j] = __dadd_rn(policies[i * D + j], sgn * t);
                }
        } else {
            const double *pl = policies + r * (M * D);
#pragma unroll
            for (int i = 0; i < M; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) W[i][j] = pl[i * D + j];
        }
        if (v2) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const double sc = inv_std[j];
#pragma unroll
                for (int i = 0; i < M; ++i) W[i][j] = __dmul_rn(W[i][j], sc);
            }
        }
        // action = W (s - mu) = W s - W mu: the constant part once per rollout
        double nbias[M];
#pragma unroll
        for (int i = 0; i < M; ++i) {
            nbias[i] = 0.0;
            if (v2) {
#pragma unroll
                for (int j = 0; j < D; ++j) nbias[i] = __builtin_fma(-W[i][j], mean[j], nbias[i]);
            }
        }

        // ---- start state ----
        double gdx, gdy, th[N], thd[N];
        if (state0) {
            gdx = state0[r];
            gdy = state0[n_roll + r];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                th[i] = state0[(int64_t)(2 + 2 * i) * n_roll + r];
                thd[i] = state0[(int64_t)(3 + 2 * i) * n_roll + r];
            }
        } else {
            gdx = gdy = TWIN ? kTwinStart : 0.0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                th[i] = TWIN ? kTwinStart : kHalfPi;
                thd[i] = TWIN ? kTwinStart : 0.0;
            }
        }

        double total = 0.0;
        bool ok = true;
        double thmax = 0.0;  // largest |theta| fed to sincos_fast
        for (int32_t t = 0; t < H; ++t) {
            thmax = sw::track_angle_range<N>(thmax, th);
            // action = W (s - mu)   (ars/environment.py:29 / :34); two partial sums
            double sm[D];
            sm[0] = gdx;
            sm[1] = gdy;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                sm[2 + 2 * i] = th[i];
                sm[3 + 2 * i] = thd[i];
            }
            double u[M];
#pragma unroll
            for (int i = 0; i < M; ++i) {
                double a0 = __builtin_fma(W[i][0], sm[0], nbias[i]), a1 = W[i][1] * sm[1];
#pragma unroll
                for (int j = 2; j < D; j += 2) {
                    a0 = __builtin_fma(W[i][j], sm[j], a0);
                    a1 = __builtin_fma(W[i][j + 1], sm[j + 1], a1);
                }
                u[i] = a0 + a1;
            }
            double rew;
            ok = (TWIN ? sw::twin_step<N>(T, gdx, gdy, th, thd, u, rew)
                       : sw::euler_step<N>(C, gdx, gdy, th, thd, u, rew)) && ok;
            total += rew;
            if (traj) {
                double *tp = traj + (int64_t)t * D * n_roll + r;
                tp[0] = gdx;
                tp[n_roll] = gdy;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    tp[(int64_t)(2 + 2 * i) * n_roll] = th[i];
                    tp[(int64_t)(3 + 2 * i) * n_roll] = thd[i];
                }
            }
            if (moments) {
                m1[0] += gdx;
                m2[0] = __builtin_fma(gdx, gdx, m2[0]);
                m1[1] += gdy;
                m2[1] = __builtin_fma(gdy, gdy, m2[1]);
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const double a = th[i] - kHalfPi;
                    m1[2 + 2 * i] += a;
                    m2[2 + 2 * i] = __builtin_fma(a, a, m2[2 + 2 * i]);
                    m1[3 + 2 * i] += thd[i];
                    m2[3 + 2 * i] = __builtin_fma(thd[i], thd[i], m2[3 + 2 * i]);
                }
            }
        }
        bool fin = isfinite(gdx) && isfinite(gdy);
#pragma unroll
        for (int i = 0; i < N; ++i) fin = fin && isfinite(th[i]) && isfinite(thd[i]);
        const bool in_range = thmax < sw::kAngleLimit;
        // an angle outside sincos_fast's range makes every later number meaningless: fail
        // loudly (NaN return + status bit) instead of returning finite garbage
#if SW_GATE_BODY
        // rollout r ^ 1 is the next lane (both are active or neither: n_roll is even)
        gate_store<1>(in_range ? total : __builtin_nan(""),
                      (ok ? 0 : SW_STATUS_SINGULAR) | (fin ? 0 : SW_STATUS_NONFINITE) | (in_range ? 0 : SW_STATUS_RANGE),
                      true, r, gate_thr, returns, status, admit);
#else
        returns[r] = in_range ? total : __builtin_nan("");
        if (status)
            status[r] = (ok ? 0 : SW_STATUS_SINGULAR) | (fin ? 0 : SW_STATUS_NONFINITE) |
                        (in_range ? 0 : SW_STATUS_RANGE);
#endif
        if (final_state) {
            final_state[r] = gdx;
            final_state[n_roll + r] = gdy;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                final_state[(int64_t)(2 + 2 * i) * n_roll + r] = th[i];
                final_state[(int64_t)(3 + 2 * i) * n_roll + r] = thd[i];
            }
        }
    }

    if (moments) {
        // fixed-order butterfly over each group of 16 lanes (deterministic); one row of
        // partial sums per 16 rollouts, the same partition the quad kernel produces
        const int64_t n_rows = (n_roll + kMomGroup - 1) / kMomGroup;
        const int64_t row = (int64_t)blockIdx.x * (kRollBlock / kMomGroup) + threadIdx.x / kMomGroup;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double a = m1[j], b = m2[j];
#pragma unroll
            for (int off = kMomGroup / 2; off > 0; off >>= 1) {
                a += __shfl_down(a, off, kMomGroup);
                b += __shfl_down(b, off, kMomGroup);
            }
            if (threadIdx.x % kMomGroup == 0 && row < n_rows) {
                moments[row * (2 * D) + j] = a;
                moments[row * (2 * D) + D + j] = b;
            }
        }
    }
