// Body of rollout_octp3_kernel, rollout_octl3_kernel and rollout_octs3_kernel (csrc/swimmer_rollout_n3.hip): the mirror-quad rollout of
// swimmer_rollout_oct3.inc with trajectory capture AND V2 moment sums, in the PACKED record form.  Included INSIDE the
// kernel's braces, with SW_OCTP_LEAN defined as 0 (rollout_octp3_kernel) or 1 (rollout_octl3_kernel: same record, same
// arithmetic, less scalar bookkeeping per step -- below, after the note on the two files).
//
// rollout_oct3_kernel<ARS, true, true> records a step with three 8-byte stores (theta and thetadot on quad-A lanes
// 0..2, Gdot on lane 0 of both quads: 24 + 24 + 16 = 64 live lanes, 128 lane slots dropped by the range check) and six
// accumulate instructions of which every lane uses at most four.  A store costs a lone wave 12-14 cycles however many
// of its lanes are live.  Here the eight state components of a rollout sit on its eight lanes, in ONE register Z:
//
//   lane of the rollout   Z holds each step                               trajectory column   shift
//   A0, A1, A2            theta of segment q (the lane's own)             2 + 2q              pi/2
//   A3 (mirror of A0)     Gdot_x (its own Pu: lane 0's, bit for bit)      0                   0
//   B0, B1, B2            thetadot of segment q, QUAD A's copy (row_ror:8) 3 + 2q             0
//   B3 (mirror of B0)     Gdot_y (its own Pu)                             1                   0
//
// so a step is recorded by one wave-wide store without a dropped lane, one m1 += X and one m2 = fma(X, X, m2) with
// X = Z - shift.  Every output has the bits of the three-store kernel: lane 3 of a quad receives what lane 0 receives
// (seg = 0, kDppNext1 = [1,2,0,1], kDppNext2 = [2,0,1,2]), the B lanes record quad A's thetadot and not their own copy
// (which differs by rounding), Z - 0.0 is exact, X on A0..A2 is that kernel's `th - pi/2`, and every accumulator sees
// the same sequence of operands.  Everything ahead of the record (lane layout, policy row, renormalisation, geometry,
// dynamics, range test, trip structure) is that kernel's, token for token.
//
// KEEP THE TWO FILES IN STEP: the shared part is a copy, because the machine code of rollout_oct3_kernel is pinned
// (tests/test_loop_placement.py) and its body cannot be restructured around a common piece.  Any fix to the shared part
// must be made in swimmer_rollout_oct3.inc AND here; tests/test_packed_capture_gpu.py (bit identity of the two
// kernels' outputs) is what notices when they drift apart.
//
// SW_OCTP_LEAN switches exactly three places of this file, marked `#if SW_OCTP_LEAN`; with 0 the text the compiler sees
// is the packed kernel's as it was, and its machine code is pinned (tests/test_packed_capture_isa.py):
//   1. where a store goes.  Packed: scalar offset soff, `soff += slab` after every store (per trip of eight a chain of
//      eight dependent s_add, and six more that rebuild base + j slab for the next trip).  Lean: the scalar offsets of a
//      trip's steps are the loop-invariant k_j = j slab, j = 1..7, pinned in SGPRs, and the inline constant 0 for the
//      trip's first step; the trip's base rides in the VECTOR offset, bumped once per trip (SW_OCTP_TRIP_END: 8 slab
//      in the main loop, 4 slab and 2 slab in the tail loops, nothing after the single last step; the amounts are
//      scalars computed ahead of the loops).  Descriptor, num_records and every address are the packed kernel's, and
//      so is the 32-bit range: the descriptor already assumes H slab < 2^32.
//   2. the step's position in its trip (SW_OCTP_STEP_AT), which selects that scalar offset.
//   3. the range test: oct3_range_test_vcc / oct3_keep_reduced_vcc (swimmer_oct3.h) -- the compare writes vcc and
//      s_cbranch_vccnz reaches the same out-of-line re-normalisation block; no s_cmp_lg_u64.
// Everything else (lane roles, Z, X = Z - shift, m1, m2, octp3_pack, the epilogue, the riding covariance tile) is one
// text for both kernels; tests/test_lean_capture_gpu.py compares their outputs bit for bit.
//
// SW_OCTP_NEXT_E (0 or 1; 1 only together with SW_OCTP_LEAN 1: rollout_octs3_kernel) switches the step itself, in the
// places marked `#if SW_OCTP_NEXT_E`; with 0 the text the compiler sees is the lean kernel's as it was, and its machine
// code is pinned as well (tests/test_lean_capture_isa.py):
//   1. the geometry: oct3_geometry_next_e forms no cos(th_i1 - th_i2);
//   2. the dynamics: oct3_dynamics_next_e takes the matrix entry Q(i+1, i+2) from lane i+1, whose Q(i, i+1) it is
//      (swimmer_oct3.h has the identity and its static_asserts): two DPP moves for three f64 instructions;
//   3. the loop: a pad of its own (oct_next_e_loop_pad()) and, with SW_OCTS_TRIP16 (swimmer_launch.h: on), a main loop
//      of sixteen steps per trip ahead of the eight-step one, with eight more pinned store offsets k8..k15.
// tests/test_neighbour_entry_gpu.py compares its outputs with the other three kernels', bit for bit.
#ifndef SW_OCTP_LEAN
#error "define SW_OCTP_LEAN as 0 or 1 before including swimmer_rollout_octp3.inc"
#endif
#ifndef SW_OCTP_NEXT_E
#error "define SW_OCTP_NEXT_E as 0 or 1 before including swimmer_rollout_octp3.inc"
#endif
#if SW_OCTP_NEXT_E && !SW_OCTP_LEAN
#error "SW_OCTP_NEXT_E is a variant of the lean mode"
#endif
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

    // the lane's trajectory cell (table above): every lane of the wave stores, nothing is dropped; the surplus
    // rollouts of the last wave rewrite rollout n_roll - 1's cells with the same values
    const bool lane3 = q == 3;
    const int column = lane3 ? (cosine ? 1 : 0) : (cosine ? cthd : cth);
    const double shift = (!cosine && !lane3) ? kHalfPi : 0.0;
    const uint32_t voff = (uint32_t)(((int64_t)column * n_roll + r) * 8);
    const uint32_t slab = (uint32_t)(D * n_roll * 8);
    const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc(
        traj, 0, (int)(uint32_t)((int64_t)H * slab), 0x00020000);
    uint32_t soff = 0;
#if SW_OCTP_LEAN
    // vrun = voff + (first step of the current trip) slab; soff = (position in the trip) slab: one of k1..k7, or 0
    uint32_t vrun = voff;
    uint32_t k1 = slab, k2 = 2 * slab, k3 = 3 * slab, k4 = 4 * slab, k5 = 5 * slab, k6 = 6 * slab, k7 = 7 * slab;
    uint32_t bump8 = 8 * slab, bump4 = 4 * slab, bump2 = 2 * slab;
    asm volatile("" : "+s"(k1), "+s"(k2), "+s"(k3), "+s"(k4), "+s"(k5), "+s"(k6), "+s"(k7));
    asm volatile("" : "+s"(bump8), "+s"(bump4), "+s"(bump2));
#if SW_OCTP_NEXT_E && SW_OCTS_TRIP16
    uint32_t k8 = 8 * slab, k9 = 9 * slab, k10 = 10 * slab, k11 = 11 * slab, k12 = 12 * slab, k13 = 13 * slab,
             k14 = 14 * slab, k15 = 15 * slab, bump16 = 16 * slab;
    asm volatile("" : "+s"(k8), "+s"(k9), "+s"(k10), "+s"(k11), "+s"(k12), "+s"(k13), "+s"(k14), "+s"(k15),
                 "+s"(bump16));
#endif
#define SW_OCTP_STEP_AT(K) soff = (K)
#define SW_OCTP_TRIP_END(BUMP) vrun += (BUMP)
    auto store_cell = [&](double v) {
        typedef int v2i __attribute__((ext_vector_type(2)));
        union { double d; v2i i; } u;
        u.d = v;
        __builtin_amdgcn_raw_buffer_store_b64(u.i, trs, (int)vrun, (int)soff, SW_TRAJ_STORE_AUX);
    };
#else
#define SW_OCTP_STEP_AT(K) (void)0
#define SW_OCTP_TRIP_END(BUMP) (void)0
    auto store_cell = [&](double v) {
        typedef int v2i __attribute__((ext_vector_type(2)));
        union { double d; v2i i; } u;
        u.d = v;
        __builtin_amdgcn_raw_buffer_store_b64(u.i, trs, (int)voff, (int)soff, SW_TRAJ_STORE_AUX);
    };
#endif

    // the angle in reduced form + the polynomial this lane currently evaluates (swimmer_oct3.h)
    const int designation = cosine ? 1 : 0;
    double thmax = 0.0, det = 1.0;
    sw::OctTrig A;
    A.r = th;
    A.kd = 0.0;
    sw::oct3_renorm(A, designation, thmax);
    double m1 = 0.0, m2 = 0.0;
    double w1 = sw::dpp_f64<sw::kDppNext1>(thd), w2 = sw::dpp_f64<sw::kDppNext2>(thd);
    double Th = __builtin_fma(V[2], th, nbias);
    Th = __builtin_fma(V[4], sw::dpp_f64<sw::kDppNext1>(th), Th);
    Th = __builtin_fma(V[6], sw::dpp_f64<sw::kDppNext2>(th), Th);
    const double hV2 = C.h * V[2], hV4 = C.h * V[4], hV6 = C.h * V[6];
#if SW_OCTP_NEXT_E
    sw::OctGeo G = sw::oct3_geometry_next_e(A), Gn;
#else
    sw::OctGeo G = sw::oct3_geometry(A), Gn;
#endif
    double magic = 6755399441055744.0;   // 1.5 * 2^52, pinned in a VGPR pair for oct3_keep_reduced
    asm volatile("" : "+v"(magic));
    auto one_step = [&](const sw::OctGeo &Gc, sw::OctGeo &Gx) {
        // theta_{t+1} needs thetadot_t only: advance the angle first and start its range test, the
        // policy's eight FMAs sit between the vector compare and the scalar branch that waits for it
        A.r = __builtin_fma(C.h, thd, A.r);
#if SW_OCTP_LEAN
        const unsigned long long outside = sw::oct3_range_test_vcc(A.r);
#else
        const unsigned long long outside = sw::oct3_range_test(A.r);
#endif
        double tq = __builtin_fma(VPu, Pu, Th);
        tq = __builtin_fma(VPv, Pv, tq);
        tq = __builtin_fma(V[3], thd, tq);
        tq = __builtin_fma(V[5], w1, tq);
        tq = __builtin_fma(V[7], w2, tq);
        Th = __builtin_fma(hV2, thd, Th);
        Th = __builtin_fma(hV4, w1, Th);
        Th = __builtin_fma(hV6, w2, Th);
#if SW_OCTP_LEAN
        sw::oct3_keep_reduced_vcc(A, thmax, magic, designation, outside);
#else
        sw::oct3_keep_reduced(A, thmax, magic, designation, outside);   // untaken branch; rare re-normalisation
#endif
#if SW_OCTP_NEXT_E
        Gx = sw::oct3_geometry_next_e(A);
        det = sw::oct3_dynamics_next_e(C, O, Gc, Pu, Pv, thd, w1, w2, tq);
#else
        Gx = sw::oct3_geometry(A);
        det = sw::oct3_dynamics(C, O, Gc, Pu, Pv, thd, w1, w2, tq);
#endif
        // the record: theta_{t+1} straight into Z (the angle itself is not carried in the loop), quad A's new
        // thetadot onto the B lanes (row_ror:8 under bank mask 0xc: lanes 8..15 of a row), Gdot onto lane 3
        const double Z = sw::octp3_pack(__builtin_fma(A.kd, sw::kPio2Hi, A.r), thd, Pu, lane3);
        const double X = Z - shift;
        m1 += X;
        m2 = __builtin_fma(X, X, m2);
        store_cell(Z);
#if !SW_OCTP_LEAN
        soff += slab;
#endif
        w1 = sw::dpp_f64<sw::kDppNext1>(thd);
        w2 = sw::dpp_f64<sw::kDppNext2>(thd);
        Pv = sw::dpp_row_f64<sw::kDppRowRor8>(Pu);
    };
    // the geometry ping-pongs between G and Gn (no register copies): an even number of steps per trip
    int32_t t = 0;
#if SW_OCTP_NEXT_E
    SW_PIN_LOOP(oct_next_e_loop_pad());
#else
    SW_PIN_LOOP(SW_OCTP_LEAN ? oct_lean_loop_pad() : oct_packed_loop_pad());
#endif
#if SW_OCTP_NEXT_E && SW_OCTS_TRIP16
    // sixteen steps per trip first (the eight-step loop below then runs at most once): measured -1.6 % on the launch
    for (; t + 16 <= H; t += 16) {
        SW_OCTP_STEP_AT(0);   one_step(G, Gn);
        SW_OCTP_STEP_AT(k1);  one_step(Gn, G);
        SW_OCTP_STEP_AT(k2);  one_step(G, Gn);
        SW_OCTP_STEP_AT(k3);  one_step(Gn, G);
        SW_OCTP_STEP_AT(k4);  one_step(G, Gn);
        SW_OCTP_STEP_AT(k5);  one_step(Gn, G);
        SW_OCTP_STEP_AT(k6);  one_step(G, Gn);
        SW_OCTP_STEP_AT(k7);  one_step(Gn, G);
        SW_OCTP_STEP_AT(k8);  one_step(G, Gn);
        SW_OCTP_STEP_AT(k9);  one_step(Gn, G);
        SW_OCTP_STEP_AT(k10); one_step(G, Gn);
        SW_OCTP_STEP_AT(k11); one_step(Gn, G);
        SW_OCTP_STEP_AT(k12); one_step(G, Gn);
        SW_OCTP_STEP_AT(k13); one_step(Gn, G);
        SW_OCTP_STEP_AT(k14); one_step(G, Gn);
        SW_OCTP_STEP_AT(k15); one_step(Gn, G);
        SW_OCTP_TRIP_END(bump16);
    }
#endif
    // eight steps per trip, as in rollout_oct3_kernel (the back edge costs a lone wave ~8-13 ns)
    for (; t + 8 <= H; t += 8) {
        SW_OCTP_STEP_AT(0);  one_step(G, Gn);
        SW_OCTP_STEP_AT(k1); one_step(Gn, G);
        SW_OCTP_STEP_AT(k2); one_step(G, Gn);
        SW_OCTP_STEP_AT(k3); one_step(Gn, G);
        SW_OCTP_STEP_AT(k4); one_step(G, Gn);
        SW_OCTP_STEP_AT(k5); one_step(Gn, G);
        SW_OCTP_STEP_AT(k6); one_step(G, Gn);
        SW_OCTP_STEP_AT(k7); one_step(Gn, G);
        SW_OCTP_TRIP_END(bump8);
    }
    for (; t + 4 <= H; t += 4) {
        SW_OCTP_STEP_AT(0);  one_step(G, Gn);
        SW_OCTP_STEP_AT(k1); one_step(Gn, G);
        SW_OCTP_STEP_AT(k2); one_step(G, Gn);
        SW_OCTP_STEP_AT(k3); one_step(Gn, G);
        SW_OCTP_TRIP_END(bump4);
    }
    for (; t + 2 <= H; t += 2) {
        SW_OCTP_STEP_AT(0);  one_step(G, Gn);
        SW_OCTP_STEP_AT(k1); one_step(Gn, G);
        SW_OCTP_TRIP_END(bump2);
    }
    SW_OCTP_STEP_AT(0);
    if (t < H) one_step(G, Gn);
#undef SW_OCTP_STEP_AT
#undef SW_OCTP_TRIP_END
    if (H > 0) th = __builtin_fma(A.kd, sw::kPio2Hi, A.r);   // the bits of the last step's Z on A0..A2
    thmax = fmax(thmax, fabs(th));

    // ---- per-rollout outputs: quad A lanes 0..2 hold (theta, thetadot), lane 3 of A the Gdot_x sums, of B Gdot_y's
    int code = ((det > 0.0) ? 0 : SW_STATUS_SINGULAR) |
               ((isfinite(th) && isfinite(thd) && isfinite(Pu) && isfinite(Pv)) ? 0 : SW_STATUS_NONFINITE) |
               ((thmax < sw::kAngleLimit) ? 0 : SW_STATUS_RANGE);
    // lane 3 computes what lane 0 computes, so with its own code and lanes 1 and 2's it has the quad's
    code |= __builtin_amdgcn_mov_dpp(code, sw::kDppNext1, 0xf, 0xf, true) |
            __builtin_amdgcn_mov_dpp(code, sw::kDppNext2, 0xf, 0xf, true);
    code |= __builtin_amdgcn_mov_dpp(code, sw::kDppRowRor8, 0xf, 0xf, true);
    const double sg_other = sw::dpp_row_f64<sw::kDppRowRor8>(m1);   // on A3: sum Gdot_y (before the reduction below)
    if (valid && !cosine && lane3) {
        const double total = __builtin_fma(C.dirx, m1, C.diry * sg_other);
        returns[r] = (code & SW_STATUS_RANGE) ? __builtin_nan("") : total;
        if (status) status[r] = code;
    }
    if (final_state && valid) {
        if (!cosine && q < 3) {
            final_state[(int64_t)cth * n_roll + r] = th;
            final_state[(int64_t)cthd * n_roll + r] = thd;
        }
        if (q == 0) final_state[(int64_t)(cosine ? 1 : 0) * n_roll + r] = Pu;
    }
    {
        __shared__ double shm[kOctBlock / kWave][16][2];
        if (!valid) m1 = m2 = 0.0;
        // sum over the 8 rollouts of the wave, per lane of the rollout: lane bits 2, 4, 5
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int off = (k == 0) ? 4 : (k == 1 ? 16 : 32);
            m1 += __shfl_xor(m1, off, kWave);
            m2 += __shfl_xor(m2, off, kWave);
        }
        if (lane < 16) {
            shm[wave][lane][0] = m1;
            shm[wave][lane][1] = m2;
        }
        __syncthreads();
        // row lanes 0..2: theta sums; 8..10: thetadot sums; 3: Gdot_x sums; 11: Gdot_y sums
        if (tid < 3) {
            double *row = moments + (int64_t)blockIdx.x * (2 * D);
            row[2 + 2 * tid] = shm[0][tid][0] + shm[1][tid][0];
            row[D + 2 + 2 * tid] = shm[0][tid][1] + shm[1][tid][1];
            row[3 + 2 * tid] = shm[0][8 + tid][0] + shm[1][8 + tid][0];
            row[D + 3 + 2 * tid] = shm[0][8 + tid][1] + shm[1][8 + tid][1];
            if (tid < 2) {
                const int src = 3 + tid * 8;
                row[tid] = shm[0][src][0] + shm[1][src][0];
                row[D + tid] = shm[0][src][1] + shm[1][src][1];
            }
        }
    }
