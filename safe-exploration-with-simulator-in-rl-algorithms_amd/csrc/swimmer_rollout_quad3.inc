// Body of rollout_quad3_kernel (csrc/swimmer_rollout_n3.hip), shared with its sw_ars_gate_f64 form and its multi-agent form
// (sw_ars_rollouts_multi_f64): included INSIDE the kernels' braces with SW_GATE_BODY 0 (the rollout kernel, token for
// token what it was; the multi-agent kernel behind swimmer_rollout_multi.inc) or 1 (the gate).
    side_flag(side);
    if (blockIdx.x >= side.first_cov_block) {   // a covariance workgroup riding along (uniform)
        side_cov_tile<8, kRollBlock>(side);
        return;
    }
    // This wave's speed IS the iteration time: first in line at the instruction arbiter when a
    // covariance workgroup of the same launch (or, multi-GPU, a collective's wave) lands on its
    // SIMD.  (Reserving the SIMD outright -- allocating all 512 registers by touching v255 / a255
    // -- measured neutral on one GPU and would serialise the covariance workgroups behind the
    // rollouts once a batch fills the chip, so it is not done.)
    __builtin_amdgcn_s_setprio(3);
    constexpr int D = 8, M = 2;
    const int lane = threadIdx.x;
    const int q = lane & 3;
    const int seg = (q == 3) ? 0 : q;              // lane 3 mirrors lane 0
    const int64_t r_raw = (int64_t)blockIdx.x * kMomGroup + (lane >> 2);
    const bool valid = r_raw < n_roll;
    const int64_t r = valid ? r_raw : n_roll - 1;  // surplus quads recompute the last rollout
    const sw::Quad3Lane L = sw::quad3_lane(seg);
    const int cth = 2 + 2 * seg, cthd = 3 + 2 * seg;

    // ---- this lane's policy row: V_i = c12 (W_{i-1} - W_i), W = (P +- nu delta) diag(inv_std)
    // (ars_agent.py:141-142, environment.py:32-34), u_{-1} = u_2 = 0 (free ends); columns in
    // this lane's rotated order [Gdx, Gdy, th_i, thd_i, th_i1, thd_i1, th_i2, thd_i2]
    const int seg1 = (seg + 1) % 3, seg2 = (seg + 2) % 3;
    const int cols[D] = {0, 1, cth, cthd, 2 + 2 * seg1, 3 + 2 * seg1, 2 + 2 * seg2, 3 + 2 * seg2};
    double V[D], nbias;   // nbias = -V . mean: tq = V . (obs - mean) without per-step subtractions
    load_policy_row<D, M, ARS>(ARS ? policies : policies + r * (M * D),
                               ARS ? deltas + (dir_begin + (r >> 1)) * (M * D) : nullptr,
                               (r & 1) ? -1.0 : 1.0, nu, mean, inv_std, C.c12, seg, cols, V, nbias);

    // ---- start state ----
    double gdx = 0.0, gdy = 0.0, th = kHalfPi, thd = 0.0;
    if (state0) {
        gdx = state0[r];
        gdy = state0[n_roll + r];
        th = state0[(int64_t)cth * n_roll + r];
        thd = state0[(int64_t)cthd * n_roll + r];
    }
    // Trajectory stores go through a buffer resource (SGPR base + per-step SGPR offset +
    // per-lane VGPR offset): one store instruction per value and one scalar add per step,
    // no per-store 64-bit address arithmetic.  The host picks this kernel only when the
    // whole trajectory buffer is < 4 GiB (32-bit offsets; out-of-range stores are dropped
    // by the hardware range check, never written elsewhere).
    const uint32_t off_th = (uint32_t)(((int64_t)cth * n_roll + r) * 8);
    const uint32_t off_thd = (uint32_t)(((int64_t)cthd * n_roll + r) * 8);
    // Gdot is replicated on every lane (each lane integrates its own copy, equal up to rounding):
    // lanes of segment 0 record (store and sum) x, the others y.  ONE store of a per-lane selected
    // value: a store costs ~16 issue cycles (measured), the select 2 x 4.4.  The rollout's
    // Gdot_y is lane 1's copy: lane 2's store is dropped by the buffer range check.
    const uint32_t kDrop = 0xfffffff0u;
    const uint32_t off_g = (q == 2) ? kDrop : (uint32_t)(((int64_t)(seg == 0 ? 0 : 1) * n_roll + r) * 8);
    const double selx = (seg == 0) ? 1.0 : 0.0, sely = 1.0 - selx;
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

    // The angle is carried in reduced form theta = r + K pi/2 (swimmer_device.h, Angle): no
    // per-step range reduction or quadrant logic in sin / cos.
    sw::Angle A = sw::angle_make(th);
    double thmax = 0.0, det = 1.0;
    asm("v_max_f64 %0, %1, |%2|" : "=v"(thmax) : "v"(thmax), "v"(th));
    double m1th = 0.0, m2th = 0.0, m1thd = 0.0, m2thd = 0.0;
    double m1g = 0.0, m2g = 0.0;   // sums of this lane's Gdot component and its square
    // neighbours' angular velocities for the next step: exchanged at the END of a step (behind
    // the stores and moment updates), so the DPP reads never wait on the Euler update that just
    // wrote them.  The neighbours' ANGLES are never exchanged: the policy is linear in them and
    // theta_j(t+1) = theta_j(t) + h thetadot_j(t), so the angle part of this lane's torque balance,
    //     Th(t) = -V . mean + sum_j V[theta_j] theta_j(t),
    // is carried along as Th(t+1) = Th(t) + sum_j (h V[theta_j]) thetadot_j(t) -- three FMAs on
    // velocities that are exchanged anyway, instead of three FMAs on angles plus four DPP moves.
    // (It also spares the per-step cancellation of V . theta against V . mean, ~1e4 against ~1
    // once the whitening is on.)
    double w1 = sw::dpp_f64<sw::kDppNext1>(thd), w2 = sw::dpp_f64<sw::kDppNext2>(thd);
    double Th = __builtin_fma(V[2], th, nbias);
    Th = __builtin_fma(V[4], sw::dpp_f64<sw::kDppNext1>(th), Th);
    Th = __builtin_fma(V[6], sw::dpp_f64<sw::kDppNext2>(th), Th);
    const double hV2 = C.h * V[2], hV4 = C.h * V[4], hV6 = C.h * V[6];
    const sw::TrigK K = sw::trig_consts();
    double magic = 6755399441055744.0;   // 1.5 * 2^52, pinned in a VGPR pair for angle_keep_reduced
    asm volatile("" : "+v"(magic));
    sw::Quad3Geo G = sw::quad3_geometry(A, K), Gn;
    // one step: consumes the geometry Gc of theta_t, produces Gx for theta_{t+1}
    auto one_step = [&](const sw::Quad3Geo &Gc, sw::Quad3Geo &Gx) {
        // this segment's torque balance c12 (u_{i-1} - u_i) = V_i . (obs - mean): the carried
        // angle part + the velocity part (the neighbours' angular velocities arrive by DPP and are
        // reused by the physics step).  One accumulator: the kernel is issue-bound, not chain-bound.
        // theta_{t+1} needs thetadot_t only: advance the angle first and start its range test; the
        // policy's eight FMAs sit between the vector compare and the scalar branch that waits for it.
        // Its sin / cos and the neighbour exchange run beside this step's solve (software pipelining
        // across steps, swimmer_quad3.h)
        A.r = __builtin_fma(C.h, thd, A.r);
        const unsigned long long outside = sw::angle_range_test(A.r);
        double tq = __builtin_fma(V[0], gdx, Th);
        tq = __builtin_fma(V[1], gdy, tq);
        tq = __builtin_fma(V[3], thd, tq);
        tq = __builtin_fma(V[5], w1, tq);
        tq = __builtin_fma(V[7], w2, tq);
        Th = __builtin_fma(hV2, thd, Th);
        Th = __builtin_fma(hV4, w1, Th);
        Th = __builtin_fma(hV6, w2, Th);
        sw::angle_keep_reduced(A, thmax, magic, outside);   // untaken branch; rare re-normalisation
        const double th_next = sw::angle_theta(A);
        Gx = sw::quad3_geometry(A, K);
        det = sw::quad3_dynamics(C, L, Gc, gdx, gdy, thd, w1, w2, tq);
        th = th_next;
        // the return comes out of the per-component sums in the epilogue (linearity), no
        // per-step reward arithmetic
        const double gsel = __builtin_fma(selx, gdx, sely * gdy);
        m1g += gsel;
        if (TRAJ) {
            store_cell(th, off_th);
            store_cell(thd, off_thd);
            store_cell(gsel, off_g);
            soff += slab;
        }
        if (MOM) {
            const double a = th - kHalfPi;
            m1th += a;
            m2th = __builtin_fma(a, a, m2th);
            m1thd += thd;
            m2thd = __builtin_fma(thd, thd, m2thd);
            m2g = __builtin_fma(gsel, gsel, m2g);
        }
        w1 = sw::dpp_f64<sw::kDppNext1>(thd);
        w2 = sw::dpp_f64<sw::kDppNext2>(thd);
    };
    // four steps per trip, the geometry ping-pongs between G and Gn (no register copies)
    int32_t t = 0;
#if SW_QUAD_UNROLL == 4
#if defined(SW_MULTI_PAD)   // a gate-multi / counted kernel of the safe batch: its own pad (swimmer_launch.h)
    SW_PIN_LOOP(SW_MULTI_PAD);
#elif defined(SW_MULTI_N)   // a multi-agent kernel: its own pad (swimmer_launch.h)
    SW_PIN_LOOP(quad_multi_loop_pad(MOM));
#else
    SW_PIN_LOOP(SW_QUAD_LOOP_PAD);
#endif
    for (; t + 4 <= H; t += 4) {
        one_step(G, Gn);
        one_step(Gn, G);
        one_step(G, Gn);
        one_step(Gn, G);
    }
#endif
    for (; t + 2 <= H; t += 2) {
        one_step(G, Gn);
        one_step(Gn, G);
    }
    if (t < H) one_step(G, Gn);
    asm("v_max_f64 %0, %1, |%2|" : "=v"(thmax) : "v"(thmax), "v"(th));
    // the joint-acceleration system is the chain's (scaled) mass matrix: positive definite for
    // every finite configuration, so its determinant can only fail to be positive once the state
    // is no longer finite -- the last step's says so
    const double detmin = det;

    // ---- per-rollout outputs (quad lanes 0..2 hold the state; lane 0 the return) ----
    int code = ((detmin > 0.0) ? 0 : SW_STATUS_SINGULAR) |
               ((isfinite(th) && isfinite(thd) && isfinite(gdx) && isfinite(gdy)) ? 0 : SW_STATUS_NONFINITE) |
               ((thmax < sw::kAngleLimit) ? 0 : SW_STATUS_RANGE);
    code |= __builtin_amdgcn_mov_dpp(code, sw::kDppNext1, 0xf, 0xf, true) |
            __builtin_amdgcn_mov_dpp(code, sw::kDppNext2, 0xf, 0xf, true);
    // sum of the rewards Gdot_t . direction (remy_swimmer_env.py:238-243), by linearity:
    // lane 0 holds sum Gdot_x, lane 1 sum Gdot_y
    const double sgy = sw::dpp_f64<sw::kDppNext1>(m1g);
#if SW_GATE_BODY
    {   // rollout r ^ 1 is the next quad: lane ^ 4
        const double total = __builtin_fma(C.dirx, m1g, C.diry * sgy);
        gate_store<4>((code & SW_STATUS_RANGE) ? __builtin_nan("") : total, code, valid && q == 0, r, gate_thr,
                      returns, status, admit);
    }
#else
    if (valid && q == 0) {
        const double total = __builtin_fma(C.dirx, m1g, C.diry * sgy);
        returns[r] = (code & SW_STATUS_RANGE) ? __builtin_nan("") : total;
        if (status) status[r] = code;
    }
#endif
    if (final_state && valid && q < 3) {
        final_state[(int64_t)cth * n_roll + r] = th;
        final_state[(int64_t)cthd * n_roll + r] = thd;
        if (q < 2) final_state[(int64_t)q * n_roll + r] = (q == 0) ? gdx : gdy;
    }
    if (MOM) {
        if (!valid) m1th = m2th = m1thd = m2thd = m1g = m2g = 0.0;
        // sum over the 16 rollouts of the wave, per segment lane: xor-butterfly over lane>>2
#pragma unroll
        for (int off = 4; off < kWave; off <<= 1) {
            m1th += __shfl_xor(m1th, off, kWave);
            m2th += __shfl_xor(m2th, off, kWave);
            m1thd += __shfl_xor(m1thd, off, kWave);
            m2thd += __shfl_xor(m2thd, off, kWave);
            m1g += __shfl_xor(m1g, off, kWave);
            m2g += __shfl_xor(m2g, off, kWave);
        }
        if (lane < 3) {
            double *row = moments + (int64_t)blockIdx.x * (2 * D);
            row[cth] = m1th;
            row[cthd] = m1thd;
            row[D + cth] = m2th;
            row[D + cthd] = m2thd;
            if (lane < 2) {
                row[lane] = m1g;
                row[D + lane] = m2g;
            }
        }
    }
