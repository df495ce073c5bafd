// Body of rollout_oct3_kernel (csrc/swimmer_rollout_n3.hip), shared with its sw_ars_gate_f64 form and its multi-agent form
// (sw_ars_rollouts_multi_f64): included INSIDE the kernels' braces with SW_GATE_BODY 0 (the rollout kernel, token for
// token what it was; the multi-agent kernel behind swimmer_rollout_multi.inc) or 1 (the gate).
    side_flag(side);
    if (blockIdx.x >= side.first_cov_block) {   // a covariance workgroup riding along (uniform)
        side_cov_tile<8, kOctBlock>(side);
        return;
    }
    __builtin_amdgcn_s_setprio(3);   // as in the quad kernel
    constexpr int D = 8, M = 2;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int q = lane & 3;
    const int seg = (q == 3) ? 0 : q;              // lane 3 of a quad mirrors lane 0
    const bool cosine = (lane & 8) != 0;           // quad B of the rollout: cosine / Gdot_y roles
    const int64_t r_raw = (int64_t)blockIdx.x * kMomGroup + wave * 8 + (lane >> 4) * 2 + ((lane >> 2) & 1);
    const bool valid = r_raw < n_roll;
    const int64_t r = valid ? r_raw : n_roll - 1;  // surplus rollouts recompute the last one
    const sw::OctLane O = sw::oct3_lane(C, seg, cosine);
    const int cth = 2 + 2 * seg, cthd = 3 + 2 * seg;

    // this lane's policy row in its rotated order [Gdx, Gdy, th_i, thd_i, th_i1, thd_i1, th_i2, thd_i2]
    const int seg1 = (seg + 1) % 3, seg2 = (seg + 2) % 3;
    const int cols[D] = {0, 1, cth, cthd, 2 + 2 * seg1, 3 + 2 * seg1, 2 + 2 * seg2, 3 + 2 * seg2};
    double V[D], nbias;
    load_policy_row<D, M, ARS>(ARS ? policies : policies + r * (M * D),
                               ARS ? deltas + (dir_begin + (r >> 1)) * (M * D) : nullptr,
                               (r & 1) ? -1.0 : 1.0, nu, mean, inv_std, C.c12, seg, cols, V, nbias);
    // Gdot in the roles: Pu = the component this quad integrates, Pv = its partner's
    const double VPu = cosine ? V[1] : V[0], VPv = cosine ? V[0] : V[1];

    double gdx = 0.0, gdy = 0.0, th = kHalfPi, thd = 0.0;
    if (state0) {
        gdx = state0[r];
        gdy = state0[n_roll + r];
        th = state0[(int64_t)cth * n_roll + r];
        thd = state0[(int64_t)cthd * n_roll + r];
    }
    double Pu = cosine ? gdy : gdx, Pv = cosine ? gdx : gdy;

    // trajectory cells through a buffer resource (as in the quad kernel); quad A records theta,
    // thetadot and Gdot_x, quad B Gdot_y; every other lane's store is dropped by the range check
    const uint32_t kDrop = 0xfffffff0u;
    const bool rec = !cosine && q < 3;
    const uint32_t off_th = rec ? (uint32_t)(((int64_t)cth * n_roll + r) * 8) : kDrop;
    const uint32_t off_thd = rec ? (uint32_t)(((int64_t)cthd * n_roll + r) * 8) : kDrop;
    const uint32_t off_g = (q == 0) ? (uint32_t)(((int64_t)(cosine ? 1 : 0) * n_roll + r) * 8) : kDrop;
    const uint32_t slab = (uint32_t)(D * n_roll * 8);
    const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc(
        traj, 0, TRAJ ? (int)(uint32_t)((int64_t)H * slab) : 0, 0x00020000);
    uint32_t soff = 0;
    auto store_cell = [&](double v, uint32_t voff) {
        typedef int v2i __attribute__((ext_vector_type(2)));
        union { double d; v2i i; } u;
        u.d = v;
        __builtin_amdgcn_raw_buffer_store_b64(u.i, trs, (int)voff, (int)soff, SW_TRAJ_STORE_AUX);
    };

    // the angle in reduced form + the polynomial this lane currently evaluates (swimmer_oct3.h)
    const int designation = cosine ? 1 : 0;
    double thmax = 0.0, det = 1.0;
    sw::OctTrig A;
    A.r = th;
    A.kd = 0.0;
    sw::oct3_renorm(A, designation, thmax);
    double m1th = 0.0, m2th = 0.0, m1thd = 0.0, m2thd = 0.0, m1g = 0.0, m2g = 0.0;
    double w1 = sw::dpp_f64<sw::kDppNext1>(thd), w2 = sw::dpp_f64<sw::kDppNext2>(thd);
    double Th = __builtin_fma(V[2], th, nbias);
    Th = __builtin_fma(V[4], sw::dpp_f64<sw::kDppNext1>(th), Th);
    Th = __builtin_fma(V[6], sw::dpp_f64<sw::kDppNext2>(th), Th);
    const double hV2 = C.h * V[2], hV4 = C.h * V[4], hV6 = C.h * V[6];
    sw::OctGeo G = sw::oct3_geometry(A), Gn;
    double magic = 6755399441055744.0;   // 1.5 * 2^52, pinned in a VGPR pair for oct3_keep_reduced
    asm volatile("" : "+v"(magic));
    auto one_step = [&](const sw::OctGeo &Gc, sw::OctGeo &Gx) {
        // theta_{t+1} needs thetadot_t only: advance the angle first and start its range test, the
        // policy's eight FMAs sit between the vector compare and the scalar branch that waits for it
        A.r = __builtin_fma(C.h, thd, A.r);
        const unsigned long long outside = sw::oct3_range_test(A.r);
        double tq = __builtin_fma(VPu, Pu, Th);
        tq = __builtin_fma(VPv, Pv, tq);
        tq = __builtin_fma(V[3], thd, tq);
        tq = __builtin_fma(V[5], w1, tq);
        tq = __builtin_fma(V[7], w2, tq);
        Th = __builtin_fma(hV2, thd, Th);
        Th = __builtin_fma(hV4, w1, Th);
        Th = __builtin_fma(hV6, w2, Th);
        sw::oct3_keep_reduced(A, thmax, magic, designation, outside);   // untaken branch; rare re-normalisation
        const double th_next = __builtin_fma(A.kd, sw::kPio2Hi, A.r);
        Gx = sw::oct3_geometry(A);
        det = sw::oct3_dynamics(C, O, Gc, Pu, Pv, thd, w1, w2, tq);
        th = th_next;
        m1g += Pu;
        if (TRAJ) {
            store_cell(th, off_th);
            store_cell(thd, off_thd);
            store_cell(Pu, off_g);
            soff += slab;
        }
        if (MOM) {
            const double a = th - kHalfPi;
            m1th += a;
            m2th = __builtin_fma(a, a, m2th);
            m1thd += thd;
            m2thd = __builtin_fma(thd, thd, m2thd);
            m2g = __builtin_fma(Pu, Pu, m2g);
        }
        w1 = sw::dpp_f64<sw::kDppNext1>(thd);
        w2 = sw::dpp_f64<sw::kDppNext2>(thd);
        Pv = sw::dpp_row_f64<sw::kDppRowRor8>(Pu);
    };
    // the geometry ping-pongs between G and Gn (no register copies): an even number of steps per trip
    int32_t t = 0;
#if defined(SW_MULTI_PAD)   // a gate-multi / counted kernel of the safe batch: its own pad (swimmer_launch.h)
    SW_PIN_LOOP(SW_MULTI_PAD);
#elif defined(SW_MULTI_N)   // a multi-agent kernel: its own pad (swimmer_launch.h)
    SW_PIN_LOOP(oct_multi_loop_pad(MOM));
#else
    SW_PIN_LOOP(oct_loop_pad(TRAJ, MOM));
#endif
#if SW_OCT_UNROLL == 8
    // eight steps per trip: the loop's back edge costs a lone wave ~8-13 ns (2 / 4 / 8 steps per trip:
    // 0.2292 / 0.2272 / 0.2250 ms per launch, each at its best loop offset; profiles/r03_t, r03_w)
    for (; t + 8 <= H; t += 8) {
        one_step(G, Gn);
        one_step(Gn, G);
        one_step(G, Gn);
        one_step(Gn, G);
        one_step(G, Gn);
        one_step(Gn, G);
        one_step(G, Gn);
        one_step(Gn, G);
    }
#endif
    for (; t + 4 <= H; t += 4) {
        one_step(G, Gn);
        one_step(Gn, G);
        one_step(G, Gn);
        one_step(Gn, G);
    }
    for (; t + 2 <= H; t += 2) {
        one_step(G, Gn);
        one_step(Gn, G);
    }
    if (t < H) one_step(G, Gn);
    thmax = fmax(thmax, fabs(th));

    // ---- per-rollout outputs: quad A lanes 0..2 hold (theta, thetadot), A lane 0 Gdot_x, B lane 0 Gdot_y
    int code = ((det > 0.0) ? 0 : SW_STATUS_SINGULAR) |
               ((isfinite(th) && isfinite(thd) && isfinite(Pu) && isfinite(Pv)) ? 0 : SW_STATUS_NONFINITE) |
               ((thmax < sw::kAngleLimit) ? 0 : SW_STATUS_RANGE);
    code |= __builtin_amdgcn_mov_dpp(code, sw::kDppNext1, 0xf, 0xf, true) |
            __builtin_amdgcn_mov_dpp(code, sw::kDppNext2, 0xf, 0xf, true);
    code |= __builtin_amdgcn_mov_dpp(code, sw::kDppRowRor8, 0xf, 0xf, true);
    const double sg_other = sw::dpp_row_f64<sw::kDppRowRor8>(m1g);   // on A: sum Gdot_y
#if SW_GATE_BODY
    {   // rollout r ^ 1 sits on lane ^ 4 (lane bit 2 selects the sign)
        const double total = __builtin_fma(C.dirx, m1g, C.diry * sg_other);
        gate_store<4>((code & SW_STATUS_RANGE) ? __builtin_nan("") : total, code, valid && !cosine && q == 0, r,
                      gate_thr, returns, status, admit);
    }
#else
    if (valid && !cosine && q == 0) {
        const double total = __builtin_fma(C.dirx, m1g, C.diry * sg_other);
        returns[r] = (code & SW_STATUS_RANGE) ? __builtin_nan("") : total;
        if (status) status[r] = code;
    }
#endif
    if (final_state && valid) {
        if (rec) {
            final_state[(int64_t)cth * n_roll + r] = th;
            final_state[(int64_t)cthd * n_roll + r] = thd;
        }
        if (q == 0) final_state[(int64_t)(cosine ? 1 : 0) * n_roll + r] = Pu;
    }
    if (MOM) {
        __shared__ double shm[kOctBlock / kWave][16][6];
        if (!valid) m1th = m2th = m1thd = m2thd = m1g = m2g = 0.0;
        // sum over the 8 rollouts of the wave, per (quad half, segment) lane: lane bits 2, 4, 5
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int off = (k == 0) ? 4 : (k == 1 ? 16 : 32);
            m1th += __shfl_xor(m1th, off, kWave);
            m2th += __shfl_xor(m2th, off, kWave);
            m1thd += __shfl_xor(m1thd, off, kWave);
            m2thd += __shfl_xor(m2thd, off, kWave);
            m1g += __shfl_xor(m1g, off, kWave);
            m2g += __shfl_xor(m2g, off, kWave);
        }
        if (lane < 16) {
            shm[wave][lane][0] = m1th;
            shm[wave][lane][1] = m2th;
            shm[wave][lane][2] = m1thd;
            shm[wave][lane][3] = m2thd;
            shm[wave][lane][4] = m1g;
            shm[wave][lane][5] = m2g;
        }
        __syncthreads();
        // row lanes 0..2: segments (quad A); row lane 0: Gdot_x sums; row lane 8: Gdot_y sums (quad B)
        if (tid < 3) {
            double *row = moments + (int64_t)blockIdx.x * (2 * D);
            row[2 + 2 * tid] = shm[0][tid][0] + shm[1][tid][0];
            row[D + 2 + 2 * tid] = shm[0][tid][1] + shm[1][tid][1];
            row[3 + 2 * tid] = shm[0][tid][2] + shm[1][tid][2];
            row[D + 3 + 2 * tid] = shm[0][tid][3] + shm[1][tid][3];
            if (tid < 2) {
                const int src = tid * 8;
                row[tid] = shm[0][src][4] + shm[1][src][4];
                row[D + tid] = shm[0][src][5] + shm[1][src][5];
            }
        }
    }
