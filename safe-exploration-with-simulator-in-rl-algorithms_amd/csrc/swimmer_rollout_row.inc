// Body of rollout_row_kernel (csrc/swimmer_rollout_row.hip), shared with its sw_ars_gate_f64 form and its multi-agent form
// (sw_ars_rollouts_multi_f64): included INSIDE the kernels' braces with SW_GATE_BODY 0 (the rollout kernel, token for
// token what it was; the multi-agent kernel behind swimmer_rollout_multi.inc) or 1 (the gate).
    side_flag(side);
    if (blockIdx.x >= side.first_cov_block) {   // a covariance workgroup riding along (uniform)
        side_cov_tile<2 * N + 2, kRowBlock>(side);
        return;
    }
    __builtin_amdgcn_s_setprio(3);   // as in the quad kernel
    constexpr int D = 2 * N + 2, M = N - 1;
    const int tid = threadIdx.x;
    const int q = tid & 15;                        // lane inside the row
    const bool owner = q < N;                      // lanes 0..N-1 own the segments' cells
    const bool cosine = q >= 8;                    // lane i + 8 mirrors lane i and evaluates the cosine
    const int seg = ((q & 7) < N) ? (q & 7) : 0;   // lanes N..7 / N+8..15 mirror lane 0 / 8
    const int64_t r_raw = (int64_t)blockIdx.x * kMomGroup + (tid >> 4);
    const bool valid = r_raw < n_roll;
    const int64_t r = valid ? r_raw : n_roll - 1;  // surplus rows recompute the last rollout
    const sw::RowLane<N> L = sw::row_lane<N>(C, seg);
    const int cth = 2 + 2 * seg, cthd = 3 + 2 * seg;

    // ---- this lane's policy row: V_i = c12 (W_{i-1} - W_i), W = (P +- nu delta) diag(inv_std)
    // (ars_agent.py:141-142, environment.py:32-34); u_{-1} = u_{n-1} = 0 (free ends)
    double V[D], nbias;   // nbias = -V . mean: tq = V . (obs - mean) without per-step subtractions
    {
        int cols[D];
#pragma unroll
        for (int j = 0; j < D; ++j) cols[j] = j;   // canonical order
        load_policy_row<D, M, ARS>(ARS ? policies : policies + r * (M * D),
                                   ARS ? deltas + (dir_begin + (r >> 1)) * (M * D) : nullptr,
                                   (r & 1) ? -1.0 : 1.0, nu, mean, inv_std, C.c12, seg, cols, V, nbias);
    }

    // ---- start state ----
    double gdx = 0.0, gdy = 0.0, th = kHalfPi, thd = 0.0;
    if (state0) {
        gdx = state0[r];
        gdy = state0[n_roll + r];
        th = state0[(int64_t)cth * n_roll + r];
        thd = state0[(int64_t)cthd * n_roll + r];
    }
    // trajectory cells through a buffer resource; lanes that own no cell get an offset
    // beyond the buffer, which the hardware range check drops
    const uint32_t slab = (uint32_t)(D * n_roll * 8);
    const uint32_t kDrop = 0xfffffff0u;
    const uint32_t off_th = (owner && valid) ? (uint32_t)(((int64_t)cth * n_roll + r) * 8) : kDrop;
    const uint32_t off_thd = (owner && valid) ? (uint32_t)(((int64_t)cthd * n_roll + r) * 8) : kDrop;
    // Gdot is replicated (bit-identical on all lanes): lane 0 stores x, lane 1 stores y, with two
    // store instructions.  (The quad kernel's per-lane select + single store has the same
    // instruction count here but measured 5 % slower: the select lands on the serial chain.)
    const uint32_t off_gx = (q == 0 && valid) ? (uint32_t)(r * 8) : kDrop;
    const uint32_t off_gy = (q == 1 && valid) ? (uint32_t)((n_roll + r) * 8) : kDrop;
    const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc(
        traj, 0, TRAJ ? (int)(uint32_t)((int64_t)H * slab) : 0, 0x00020000);
    uint32_t soff = 0;
    auto store_cell = [&](double v, uint32_t voff) {
        typedef int v2i __attribute__((ext_vector_type(2)));
        union { double d; v2i i; } u;
        u.d = v;
        __builtin_amdgcn_raw_buffer_store_b64(u.i, trs, (int)voff, (int)soff, SW_TRAJ_STORE_AUX);
    };

    double thmax = 0.0, rq_last = 1.0;
    double m1th = 0.0, m2th = 0.0, m1thd = 0.0, m2thd = 0.0;
    double sgx = 0.0, sgy = 0.0, qgx = 0.0, qgy = 0.0;   // sums of Gdot and Gdot^2 over the steps
    // theta = r + K pi/2 and the polynomial this lane evaluates of r (swimmer_oct3.h, OctTrig)
    const int designation = cosine ? 1 : 0;
    sw::OctTrig A;
    A.r = th;
    A.kd = 0.0;
    sw::oct3_renorm(A, designation, thmax);
    // one step: policy + physics (swimmer_row.h; the other segments' angles and angular velocities are
    // read straight out of their lanes by fused broadcast-FMAs), then the step's records
    auto one_step = [&](auto slow) {
        const double rq = sw::row_step<N, decltype(slow)::value>(C, L, V, nbias, cosine, designation, gdx, gdy,
                                                                 A, th, thd, thmax);
        rq_last = rq;   // the system is the chain's mass matrix: a pivot can only fail to be positive once the
                        // state is no longer finite, and then the last step's says so
        // the return comes out of the per-component sums in the epilogue (linearity)
        sgx += gdx;
        sgy += gdy;
        if (TRAJ) {
            store_cell(th, off_th);
            store_cell(thd, off_thd);
            store_cell(gdx, off_gx);
            store_cell(gdy, off_gy);
            soff += slab;
        }
        if (MOM) {
            const double a = th - kHalfPi;
            m1th += a;
            m2th = __builtin_fma(a, a, m2th);
            m1thd += thd;
            m2thd = __builtin_fma(thd, thd, m2thd);
            qgx = __builtin_fma(gdx, gdx, qgx);
            qgy = __builtin_fma(gdy, gdy, qgy);
        }
    };
    // Range check once per trip of four steps (the mirror-quad kernel's per-step asm check would cost
    // registers this kernel does not have at n >= 6): a trip whose angles move at most kTripSlack runs
    // unchecked after one re-normalisation at its start if needed -- r ends at most that far past pi/4,
    // where the polynomials are still accurate to 2.5e-16 (swimmer_oct3.h); a faster trip runs in the
    // second loop, which checks inside every step (exact for any angular velocity).  What thetadot GAINS inside
    // an unchecked trip is not in that bound: an angle travels up to 6 h^2 |thetadotdot| further (0.06 rad at
    // 10 000 rad/s^2) before the next trip start sees the speed.  The polynomials degrade smoothly out there --
    // 2.0e-16 at pi/4 + 0.04, 1.7e-15 at + 0.10, 9e-14 at + 0.25 (tests/test_trig_range.py) -- and rollouts with
    // first-step accelerations of 3 000 ... 20 000 rad/s^2 stay within 1e-6 (relative) of the oracle
    // (tests/test_hip_parity.py::test_violent_accelerations_inside_an_unchecked_trip).  One step per loop
    // body either way: unrolled, n >= 6 would leave the 256 architectural registers.
    auto too_fast = [&]() -> bool {
        return __any((4.0 * C.h) * fabs(thd) > sw::kTripSlack);
    };
    int32_t t = 0;
#if defined(SW_MULTI_PAD)   // a gate-multi / counted kernel of the safe batch: its own pad (swimmer_launch.h)
    SW_PIN_LOOP(SW_MULTI_PAD);
#elif defined(SW_MULTI_N)   // a multi-agent kernel: its own pad (swimmer_launch.h)
    SW_PIN_LOOP(row_multi_loop_pad(N, MOM));
#else
    SW_PIN_LOOP(row_loop_pad(N, TRAJ, MOM));
#endif
    while (t < H) {   // two loops, not one loop with two bodies: merged, the compiler reconciles the bodies'
                      // register assignments with copies on the common path (profiles/r03_g_ab_range_check_variants.log)
        while (t < H) {                              // unchecked trips of (up to) four steps
            if (__builtin_expect(too_fast(), 0)) break;
            const double reach = __builtin_fma(4.0 * C.h, fabs(thd), fabs(A.r));
            if (__builtin_expect(__any(reach > sw::kPio4), 0)) sw::oct3_renorm(A, designation, thmax);
            const int32_t t_end = min(H, t + 4);
#pragma unroll 1
            for (; t < t_end; ++t) one_step(std::false_type{});
        }
#pragma unroll 1
        for (; t < H && too_fast(); ++t) one_step(std::true_type{});   // checks inside every step
    }

    thmax = fmax(thmax, fabs(th));
    // ---- per-rollout outputs ----
    {
        double bad[N], big[N], piv[N];
        const bool fin = isfinite(th) && isfinite(thd) && isfinite(gdx) && isfinite(gdy);
        sw::RowGather<N>::run(fin ? 0.0 : 1.0, bad);
        sw::RowGather<N>::run(thmax, big);
        sw::RowGather<N>::run(rq_last, piv);      // every segment lane's last 1 / pivot
        double nbad = 0.0, tmax = 0.0, pmin = 1.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            nbad += bad[k];
            tmax = fmax(tmax, big[k]);
            pmin = fmin(pmin, piv[k]);
        }
        const int code = ((pmin > 0.0) ? 0 : SW_STATUS_SINGULAR) |
                         ((nbad == 0.0) ? 0 : SW_STATUS_NONFINITE) |
                         ((tmax < sw::kAngleLimit) ? 0 : SW_STATUS_RANGE);
#if SW_GATE_BODY
        {   // rollout r ^ 1 is the next row of 16 lanes: lane ^ 16
            const double total = __builtin_fma(C.dirx, sgx, C.diry * sgy);
            gate_store<16>((code & SW_STATUS_RANGE) ? __builtin_nan("") : total, code, valid && q == 0, r,
                           gate_thr, returns, status, admit);
        }
#else
        if (valid && q == 0) {
            // sum of the rewards Gdot_t . direction (remy_swimmer_env.py:238-243), by linearity
            const double total = __builtin_fma(C.dirx, sgx, C.diry * sgy);
            returns[r] = (code & SW_STATUS_RANGE) ? __builtin_nan("") : total;
            if (status) status[r] = code;
        }
#endif
    }
    if (final_state && valid && owner) {
        final_state[(int64_t)cth * n_roll + r] = th;
        final_state[(int64_t)cthd * n_roll + r] = thd;
        if (q < 2) final_state[(int64_t)q * n_roll + r] = (q == 0) ? gdx : gdy;
    }
    if (MOM) {
        __shared__ double shm[kRowBlock / kWave][16][6];
        double m1g = (q == 0) ? sgx : sgy, m2g = (q == 0) ? qgx : qgy;   // lane 0: x, lane 1: y
        if (!valid || !owner) m1th = m2th = m1thd = m2thd = m1g = m2g = 0.0;
        // sum over the 4 rows of the wave (lane bits 4, 5), then over the 4 waves through LDS
#pragma unroll
        for (int off = 16; off < kWave; off <<= 1) {
            m1th += __shfl_xor(m1th, off, kWave);
            m2th += __shfl_xor(m2th, off, kWave);
            m1thd += __shfl_xor(m1thd, off, kWave);
            m2thd += __shfl_xor(m2thd, off, kWave);
            m1g += __shfl_xor(m1g, off, kWave);
            m2g += __shfl_xor(m2g, off, kWave);
        }
        const int wv = tid / kWave, ln = tid % kWave;
        if (ln < 16) {
            shm[wv][ln][0] = m1th;
            shm[wv][ln][1] = m2th;
            shm[wv][ln][2] = m1thd;
            shm[wv][ln][3] = m2thd;
            shm[wv][ln][4] = m1g;
            shm[wv][ln][5] = m2g;
        }
        __syncthreads();
        if (tid < N) {
            double acc[6];
#pragma unroll
            for (int v = 0; v < 6; ++v)
                acc[v] = (shm[0][tid][v] + shm[1][tid][v]) + (shm[2][tid][v] + shm[3][tid][v]);
            double *row = moments + (int64_t)blockIdx.x * (2 * D);
            row[2 + 2 * tid] = acc[0];
            row[D + 2 + 2 * tid] = acc[1];
            row[3 + 2 * tid] = acc[2];
            row[D + 3 + 2 * tid] = acc[3];
            if (tid < 2) {
                row[tid] = acc[4];
                row[D + tid] = acc[5];
            }
        }
    }
