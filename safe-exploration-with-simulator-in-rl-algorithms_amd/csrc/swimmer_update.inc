// Body of ars_update_kernel (csrc/swimmer_update.hip), shared with ars_update_multi_kernel: included INSIDE the
// kernels' braces (the single-agent kernel token for token what it was; the multi kernel first points deltas, policy,
// running, mean, inv_std, sigma_out and the GatherView gv at the slices of the agent its workgroup serves).
    __shared__ double sh2[BLOCK / kWave][2];
    __shared__ double rp_s[kUpdMaxDirs], rm_s[kUpdMaxDirs];   // r+ and r- of every direction
    __shared__ unsigned char flag[kUpdMaxDirs];
    const int e = blockIdx.x;
    if (e < md) {
        const bool select = top_b > 0 && top_b < n_dir;
        const bool in_lds = n_dir <= kUpdMaxDirs;
        // one round of global loads: returns -> LDS, this workgroup's delta column -> registers
        constexpr int kMaxPer = (kUpdMaxDirs + BLOCK - 1) / BLOCK;
        double dcol[kMaxPer];
        if (in_lds) {
#pragma unroll
            for (int q = 0; q < kMaxPer; ++q) {
                const int32_t i = threadIdx.x + q * BLOCK;
                dcol[q] = (i < n_dir) ? deltas[(int64_t)i * md + e] : 0.0;
            }
            for (int32_t i = threadIdx.x; i < n_dir; i += BLOCK) {
                rp_s[i] = ret_at(gv, i, 0);
                rm_s[i] = ret_at(gv, i, 1);
            }
            __syncthreads();
            if (select && n_dir <= kTopBSortDirs) {
                // Up to 2048 directions: a bitonic sort of (key, index) in LDS, best first -- key = max(r+, r-)
                // descending, ties to the higher index, NaN keys first (np.argsort puts NaN last and the reference
                // reverses it, ars_agent.py:105-108).  log2(P) (log2(P) + 1) / 2 compare-exchange stages of P / 2
                // pairs each (45 stages at 512 directions: ~4 us) instead of N^2 / BLOCK comparisons per thread with
                // the key list re-read for every direction (~25 us on the critical path between two rollout launches).
                __shared__ double skey[kTopBSortDirs];
                __shared__ uint16_t sidx[kTopBSortDirs];
                uint32_t P2 = 2;
                while (P2 < (uint32_t)n_dir) P2 <<= 1;
                for (uint32_t i = threadIdx.x; i < P2; i += BLOCK) {
                    double k = -HUGE_VAL;
                    if (i < (uint32_t)n_dir) {
                        // NOT fmax: Python's max(a, b) = (b > a) ? b : a (safe_ars / ars_agent sort_directions)
                        const double a = rp_s[i], b = rm_s[i];
                        k = (b > a) ? b : a;
                        k = (k != k) ? HUGE_VAL : k;
                    }
                    skey[i] = k;
                    sidx[i] = (uint16_t)i;
                }
                __syncthreads();
                for (uint32_t k = 2; k <= P2; k <<= 1) {
                    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                        for (uint32_t t = threadIdx.x; t < P2 / 2; t += BLOCK) {
                            const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
                            const double ka = skey[lo], kb = skey[hi];
                            const uint32_t ia = sidx[lo], ib = sidx[hi];
                            // a goes before b?  padding (index >= n_dir) always goes last
                            const bool a_first = (ia < (uint32_t)n_dir) &&
                                                 ((ib >= (uint32_t)n_dir) || ka > kb || (ka == kb && ia > ib));
                            const bool best_first = (lo & k) == 0;     // direction of this bitonic block
                            if (a_first != best_first) {
                                skey[lo] = kb;
                                skey[hi] = ka;
                                sidx[lo] = (uint16_t)ib;
                                sidx[hi] = (uint16_t)ia;
                            }
                        }
                        __syncthreads();
                    }
                }
                for (uint32_t pos = threadIdx.x; pos < P2; pos += BLOCK) {
                    const uint32_t i = sidx[pos];
                    if (i < (uint32_t)n_dir) flag[i] = (int64_t)pos < top_b;
                }
                __syncthreads();
            } else if (select) {
                for (int32_t i = threadIdx.x; i < n_dir; i += BLOCK) {
                    const double ki = fmax(rp_s[i], rm_s[i]);
                    int32_t rank = 0;
                    for (int32_t j = 0; j < n_dir; ++j) {
                        const double kj = fmax(rp_s[j], rm_s[j]);
                        rank += (kj > ki) || (kj == ki && j > i);
                    }
                    flag[i] = rank < top_b;
                }
                __syncthreads();
            }
        }
        auto rplus = [&](int32_t i) { return in_lds ? rp_s[i] : ret_at(gv, i, 0); };
        auto rminus = [&](int32_t i) { return in_lds ? rm_s[i] : ret_at(gv, i, 1); };
        auto dir_used = [&](int32_t i) -> bool {
            if (!select) return true;
            return in_lds ? (flag[i] != 0) : rank_used_global(gv, n_dir, top_b, i);
        };
        // np.std(used_rewards): two-pass, ddof = 0 (ars_agent.py:123)
        double s = 0.0, cnt = 0.0;
        for (int32_t i = threadIdx.x; i < n_dir; i += BLOCK)
            if (dir_used(i)) {
                s += rplus(i) + rminus(i);
                cnt += 2.0;
            }
        block_sum2<BLOCK>(s, cnt, sh2);
        const double mu = s / cnt;
        double v = 0.0, g = 0.0;
        if (in_lds) {
#pragma unroll   // static index into dcol[] (a runtime index would send it to scratch)
            for (int q = 0; q < kMaxPer; ++q) {
                const int32_t i = threadIdx.x + q * BLOCK;
                if (i < n_dir && dir_used(i)) {
                    const double rp = rp_s[i], rm = rm_s[i];
                    const double a = rp - mu, c = rm - mu;
                    v += a * a + c * c;
                    g = __builtin_fma(rp - rm, dcol[q], g);
                }
            }
        } else {
            for (int32_t i = threadIdx.x; i < n_dir; i += BLOCK)
                if (dir_used(i)) {
                    const double rp = rplus(i), rm = rminus(i);
                    const double a = rp - mu, c = rm - mu;
                    v += a * a + c * c;
                    g = __builtin_fma(rp - rm, deltas[(int64_t)i * md + e], g);
                }
        }
        block_sum2<BLOCK>(v, g, sh2);
        if (threadIdx.x == 0) {
            const double sigma = sqrt(v / cnt);
            // divisor: b as given (ars_agent.py:128: all directions used, b only divides), or with
            // a true top-b truncation the number of directions used, len(order) (safe_ars/ars.py:64)
            const double div = (top_b > 0) ? 0.5 * cnt : b;
            const double grad = g / (div * sigma);
            policy[e] = policy[e] + alpha * grad;           // ars_agent.py:130
            if (e == 0 && sigma_out) *sigma_out = sigma;
        }
    } else if (running != nullptr) {
        // V2 statistics over every state seen since training began (np.mean / np.cov with
        // ddof = 1, ars_agent.py:179-182).  The reference recomputes them two-pass over the
        // whole (ever-growing) list; here `running` = {n, mean - c, M2 = sum (x - mean)^2} and
        // each iteration's batch is MERGED into it (Chan et al.): the batch's own mean and M2
        // come from its sums about the pivot c (reset state; every rollout starts there, so
        // |mean_b - c| is never large against the batch's spread), and the merge itself adds
        // non-negative terms only -- no cancellation that grows with the length of training.
        // The workgroup's 256 threads form G = 256 / 2d row groups x 2d columns: thread (rg, j) sums
        // column j over the rows whose GLOBAL index (rank-major) is congruent to rg mod G, in
        // ascending order, eight loads in flight per round (one round up to 8 G rows: 128 rows for
        // n = 3) -- the loop used to run over 4 row groups only and paid one memory latency per 16
        // rows, 4 rounds at 512 directions.  The G partial sums are added in ascending group
        // order.  Global row indices make the grouping -- and every bit of the result --
        // independent of the world size for row-aligned shards, and identical on every rank.
        constexpr int kMaxCols = 2 * (2 * SW_MAX_SEGMENTS + 2);     // 2d <= 36
        constexpr int kMaxGroups = BLOCK / 12;                  // 2d >= 12 (n = 2): G <= 21 (16 for n = 3)
        __shared__ double part[kMaxGroups][kMaxCols];
        __shared__ double bsum[kMaxCols];
        const int cols = 2 * d, G = BLOCK / cols;
        const int rg = threadIdx.x / cols, j = threadIdx.x - rg * cols;
        const int32_t total = gv.world * gv.rows_chunk;
        if (rg < G) {
            double acc = 0.0;
            for (int32_t g0 = rg; g0 < total; g0 += 8 * G) {
                double v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int32_t g = g0 + q * G;
                    v[q] = 0.0;
                    if (g < total) {
                        const int32_t r = g / gv.rows_chunk, row = g - r * gv.rows_chunk;
                        v[q] = gv.mom_base[r * gv.seg_len + (int64_t)row * cols + j];
                    }
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) acc += v[q];
            }
            part[rg][j] = acc;
        }
        __syncthreads();
        if (threadIdx.x < cols) {
            double t = part[0][threadIdx.x];
            for (int g = 1; g < G; ++g) t += part[g][threadIdx.x];
            bsum[threadIdx.x] = t;
        }
        __syncthreads();
        const double n0 = running[0], n1 = n0 + n_new;
        if (threadIdx.x < d && n_new > 0.0) {
            const int c_ = threadIdx.x;
            const double s1 = bsum[c_], s2 = bsum[d + c_];
            const double mb = s1 / n_new;                       // batch mean - c
            const double m2b = __builtin_fma(-s1, mb, s2);      // batch sum (x - mean_b)^2
            const double mr = running[1 + c_], m2 = running[1 + d + c_];
            const double delta = mb - mr;
            const double mr1 = __builtin_fma(delta, n_new / n1, mr);
            const double m21 = (m2 + m2b) + delta * delta * (n0 * (n_new / n1));
            running[1 + c_] = mr1;
            running[1 + d + c_] = m21;
            const double c = (c_ >= 2 && (c_ & 1) == 0) ? kHalfPi : 0.0;
            mean[c_] = c + mr1;
            inv_std[c_] = 1.0 / sqrt(m21 / (n1 - 1.0));          // diag(cov) ** -0.5
        }
        __syncthreads();
        if (threadIdx.x == 0) running[0] = n1;
    }
