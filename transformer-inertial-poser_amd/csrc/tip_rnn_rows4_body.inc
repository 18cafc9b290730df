    // abl: MEASUREMENT-ONLY ablations (wrong results), TIP_RNN_ABLATE: 1 = polls never wait, 2 = no MFMAs
    constexpr int R = 512, KB = R / 16, CLUSTER = 32 / WAVES, LD = kQ4LD;
    constexpr int THREADS = WAVES * 64, PL = 8 / WAVES;            // 16-byte pieces of a pulled tile per thread: 1 (8 waves) or 2 (4 waves)
    static_assert(WAVES == 8 || WAVES == 4, "cluster of 4 or 8 members");
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [2 buffers][NT tiles][4 rows][LD]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    if (TRACE && blockIdx.x == 0 && tid == 0) g_rnn_trace[3] = __builtin_amdgcn_s_memtime();   // kernel entry
    // cluster membership: members are 8 workgroup ids apart — one XCD as workgroups are observed to be dealt (verified below,
    // never assumed); the grid is whole rounds of 8 clusters, the clusters past `ngroups` have nothing to do
    const int cid = (blockIdx.x >> 3) % CLUSTER, group = (blockIdx.x & 7) + 8 * ((blockIdx.x >> 3) / CLUSTER);
    if (group >= ngroups) return;
    const int nb = cid * WAVES + wave;                            // global 16-column block of this wave
    const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(hall, 0, hall_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ih), 0, hall_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(BWD ? gate : ih), 0, hall_bytes, 0x00020000);
    // TIP_OPT_FAULT_INJECT: this member never arrives
    const bool dead = (gd.fault & 2) && group == 0 && cid == 1;
    if (dead) return;
    const unsigned spin_big = guard_spin_limit(gd.fault, 1u << 22), spin_pull = guard_spin_limit(gd.fault, 1u << 20);

    // this thread's 16-byte pieces of a pulled tile: row prow, columns pcol + 4 i (i < PL)
    const int prow = tid / (THREADS / 4), pcol = (tid % (THREADS / 4)) * (4 * PL);
    const int tpg = (ntiles + ngroups - 1) / ngroups;             // tiles per cluster
    const unsigned rowbytes = (unsigned)T * R * 4;
    int vpull[NT], vout[NT];
    auto set_tiles = [&](int q0) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            int tile = group + ngroups * (q0 + n);
            if (q0 + n >= tpg || tile >= ntiles) tile = ntiles;   // past the batch: rows >= B, out of the descriptor's range
            vpull[n] = (int)((unsigned)(tile * kQ4Rows + prow) * rowbytes + (unsigned)pcol * 4u);
            vout[n] = (int)((unsigned)(tile * kQ4Rows + lg) * rowbytes + (unsigned)(nb * 16 + l15) * 4u);
        }
    };
    // The input term (and the backward's gate) of step t + 1 is requested during step t's MFMA phase, AFTER its pull: vector
    // memory returns in order, so an HBM-latency load issued in front of the poll loads would hold every one of them back.
    float ihn[NT], gn[NT];
    auto request_inputs = [&](int te_) {
        const int so = te_ * (R * 4);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            ihn[n] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(irs, vout[n], so, Ctl::kIhAux));
            gn[n] = BWD ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grs, vout[n], so, 0)) : 0.f;
        }
    };
    // The rows the producers are about to write sit in HBM / Infinity Cache (the encoder armed them with the sentinel long
    // ago): a 64-byte store then allocates a PARTIALLY valid line in L2, and the first poll of that line waits for its fill
    // from memory.  Each member therefore touches (one 16-byte load per thread and tile, result unused) the rows of step
    // t + 2 during step t: the producers' stores then hit valid lines and the polls are plain L2 hits.
    u32x4 pfv[NT];
    auto touch_rows = [&](int te_) {
        const int so = te_ * (R * 4);
#pragma unroll
        for (int n = 0; n < NT; ++n) pfv[n] = __builtin_amdgcn_raw_buffer_load_b128(hrs, vpull[n], so, 16);
    };
    auto retire_touch = [&]() {
#pragma unroll
        for (int n = 0; n < NT; ++n) asm volatile("" :: "v"(pfv[n]));
    };
    // Step 0 of the first batch needs no W_hh (h_{-1} = 0): its input term and row touches are requested IN FRONT of the 256-KB
    // weight load (vector memory returns in order), so that step is over when the weights land instead of starting then.
    // (Ctl::kRound — the one-launch round, tip_round.hip: the input terms are produced INSIDE this launch; both requests wait for them below)
    set_tiles(0);
    if constexpr (!Ctl::kRound) {
    request_inputs(BWD ? T - 1 : 0);
    touch_rows(BWD ? T - 1 : 0);
    }
    // W_hh slice -> registers, once: all 32 k-blocks of this wave's 16 columns (in flight during the exchange below)
    float4 wreg[KB];
    {
        const float4* wf = reinterpret_cast<const float4*>(whh_frag) + (size_t)nb * KB * 64 + lane;
#pragma unroll
        for (int k = 0; k < KB; ++k) wreg[k] = wf[(size_t)k * 64];
    }
    // same-XCD fast path, verified at run time through launch-tagged exchange words (see rnn_resident_kernel)
    __shared__ int s_same_xcd;
    if (tid == 0 && dead) s_same_xcd = 0;
    if (tid == 0 && !dead) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 0xf;
        const unsigned mine = (etag << 5) | (xcc + 1u);
        __hip_atomic_store(flags + group * CLUSTER + cid, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool same = true;
        for (int m = 0; m < CLUSTER; ++m) {
            unsigned v = 0;
            bool here = false;
            for (unsigned spins = 0; spins < spin_big; ++spins) {
                v = __hip_atomic_load(flags + group * CLUSTER + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                here = (v >> 5) == etag && (v & 31u) != 0u;
                if (here) break;
                __builtin_amdgcn_s_sleep(1);
            }
            if (!here) note_spin_timeout(gd.err);
            if constexpr (Ctl::kRound) if (!here) ctl.member_lost(m);
            same &= (v == mine);
        }
        if constexpr (Ctl::kRound)   // bit 1: the tile's input terms never became ready (bounded wait, the same give-up path)
            s_same_xcd = ((same && !(gd.fault & 8)) ? 1 : 0) | (ctl.inputs_ready(group, spin_big, gd) ? 0 : 2);
        else
        s_same_xcd = (same && !(gd.fault & 8)) ? 1 : 0;
    }
    __syncthreads();
    bool same_xcd_;
    if constexpr (Ctl::kRound) same_xcd_ = (s_same_xcd & 1) != 0;
    else same_xcd_ = s_same_xcd != 0;
    const bool same_xcd = same_xcd_;
    if (TRACE && blockIdx.x == 0 && tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        g_rnn_trace[7] = __builtin_amdgcn_s_memtime();   // XCC exchange done, W_hh slice in registers
    }
    const int aoff = (lane & 3) * LD + lg * 4;                    // this lane's A operand: row lane & 3, k = 16 kb + 4 lg ..
    const int lds_w = prow * LD + pcol;                            // where this thread's 16 bytes of a pulled tile go
    bool poisoned = false;                                         // (wave-uniform)
    if constexpr (Ctl::kRound) {
        // the polling wave has joined the barrier above: every wave may now load the input terms (agent-coherent loads, Ctl::kIhAux)
        request_inputs(0);
        touch_rows(0);
        if (s_same_xcd & 2) {   // lost inputs: everything this member produces is the canonical NaN from step 0 on
            poisoned = true;
#pragma unroll
            for (int n = 0; n < NT; ++n) ihn[n] = __uint_as_float(kPoisonBits);
        }
    }
    if (TRACE && tid == 0 && blockIdx.x < 512) {                   // which workgroups share a CU (tools/rnn_hwid.py: ids j and j + 32 of an XCD)
        unsigned hwid, xccid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xccid));
        g_rnn_trace[1024 + blockIdx.x] = (unsigned long long)hwid | ((unsigned long long)(xccid & 0xf) << 32);
    }

    u32x4 pv[PL];                                                  // early-requested pull of the next tile (NT > 1)
#pragma unroll
    for (int i = 0; i < PL; ++i) pv[i] = (u32x4){kRnnSentinel, kRnnSentinel, kRnnSentinel, kRnnSentinel};
    // The whole step loop exists twice, for partners on this XCD (plain stores) and elsewhere (sc1 stores, paced polls): as a
    // branch around the store inside the loop, the structurised control flow has a path without a store, and the compiler then
    // cannot count the stores in flight — every wait behind it (the next tile's early pull) became vmcnt(0), i.e. waited for
    // the store's acknowledgement.
    auto run_steps = [&](auto same_tag) {
        constexpr bool SAME_XCD = decltype(same_tag)::value;
        for (int q0 = dead ? tpg : 0; q0 < tpg; q0 += NT) {
            if (q0 > 0) {
                set_tiles(q0);
                request_inputs(BWD ? T - 1 : 0);
                touch_rows(BWD ? T - 1 : 0);
            }
            retire_touch();
            if (T > 1) touch_rows(BWD ? T - 2 : 1);
    #pragma unroll 1
            for (int t = 0; t < T; ++t) {
                const int te = BWD ? T - 1 - t : t;        // time index this step produces
                const int tp = BWD ? te + 1 : te - 1;      // time index of the state it consumes
                float ihv[NT], gv[NT];
    #pragma unroll
                for (int n = 0; n < NT; ++n) ihv[n] = ihn[n], gv[n] = gn[n];
                float* buf = smem + (t & 1) * (NT * kQ4Rows * LD);
                const int so_out = te * (R * 4);
                // Tile by tile: pull -> LDS -> barrier -> MFMAs -> tanh -> store.  With several tiles per cluster (NT > 1) the pull of the
                // NEXT tile (the first tile's of the next step behind the last one) is requested in front of this tile's matrix phase:
                // that tile's state was stored one to NT - 1 matrix phases ago, so the request finds it in L2 and its round trip runs
                // under the MFMAs; only a request that still saw a sentinel falls back to the polling loop.  Pulling every tile at the
                // top of the step left the last tile's hop exposed on every step (first version); pulling tile by tile WITHOUT the early
                // request exposed an L2 round trip + LDS write + barrier per tile (B = 1024: 251 us against 235).  One barrier per
                // tile and step: the tile buffers alternate with t, so nobody overwrites what a slow wave still reads.  Same
                // arithmetic per tile, bit-identical.
    #pragma unroll
                for (int n = 0; n < NT; ++n) {
                    if (t > 0) {
                        // pull h_{t-1}: 16 bytes per thread, sc1 loads (agent-scope coherent); the wave re-asks while any of its lanes
                        // still sees a sentinel word
                        const int so = tp * (R * 4);
                        u32x4 v[PL];
                        bool pend = true;
                        if (NT > 1) {
                            pend = false;
    #pragma unroll
                            for (int i = 0; i < PL; ++i) {
                                v[i] = pv[i];
                                pend |= v[i].x == kRnnSentinel || v[i].y == kRnnSentinel || v[i].z == kRnnSentinel || v[i].w == kRnnSentinel;
                            }
                        }
                        bool gave_up = false;
                        if (NT == 1 || (__builtin_amdgcn_ballot_w64(pend) != 0 && !(abl & 1))) {   // (wave-uniform)
                            gave_up = true;
                            const unsigned pull_lim = poisoned ? 1u : spin_pull;
                            for (unsigned spins = 0; spins < pull_lim; ++spins) {
                                pend = false;
                                asm volatile("" ::: "memory");   // the addresses are loop invariant: without this the optimiser polls a register
    #pragma unroll
                                for (int i = 0; i < PL; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b128(hrs, vpull[n] + 16 * i, so, 16);
    #pragma unroll
                                for (int i = 0; i < PL; ++i)
                                    pend |= v[i].x == kRnnSentinel || v[i].y == kRnnSentinel || v[i].z == kRnnSentinel || v[i].w == kRnnSentinel;
                                if (TRACE && n == 0 && !(abl & 128) && blockIdx.x == 0 && tid == 0 && t < 24) {
                                    if (spins == 0) g_rnn_trace[160 + (t - 1) * 4 + 0] = __builtin_amdgcn_s_memtime();
                                    g_rnn_trace[160 + (t - 1) * 4 + 3] = spins + 1;
                                }
                                if (__builtin_amdgcn_ballot_w64(pend) == 0 || (abl & 1)) { gave_up = false; break; }
                                if (!SAME_XCD) __builtin_amdgcn_s_sleep(2);   // cross-XCD polls travel the fabric: pace them
                            }
                        }
                        if (TRACE && n == 0 && !(abl & 128) && blockIdx.x == 0 && tid == 0 && t < 24) g_rnn_trace[160 + (t - 1) * 4 + 1] = __builtin_amdgcn_s_memtime();
                        if (TRACE && n == 0 && (abl & 128) && ((abl >> 8) & 7) == 3 && blockIdx.x == 0 && tid == 0 && t < 64) g_rnn_trace[t * 4 + 1] = __builtin_amdgcn_s_memtime();
                        if (gave_up) {   // (wave-uniform)
                            if (!poisoned && lane == 0) note_spin_timeout(gd.err);
                            poisoned = true;
    #pragma unroll
                            for (int i = 0; i < PL; ++i) {   // what never arrived becomes NaN, not the sentinel
                                if (v[i].x == kRnnSentinel) v[i].x = kPoisonBits;
                                if (v[i].y == kRnnSentinel) v[i].y = kPoisonBits;
                                if (v[i].z == kRnnSentinel) v[i].z = kPoisonBits;
                                if (v[i].w == kRnnSentinel) v[i].w = kPoisonBits;
                            }
                        }
    #pragma unroll
                        for (int i = 0; i < PL; ++i) *reinterpret_cast<u32x4*>(buf + n * kQ4Rows * LD + lds_w + 4 * i) = v[i];
                        if (TRACE && n == 0 && !(abl & 128) && blockIdx.x == 0 && tid == 0 && t < 24) {
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            g_rnn_trace[160 + (t - 1) * 4 + 2] = __builtin_amdgcn_s_memtime();
                        }
                        __syncthreads();
                    }
                    if (TRACE && n == 0 && !(abl & 128) && blockIdx.x == 0 && tid == 0 && t < 64) g_rnn_trace[t * 4 + 0] = __builtin_amdgcn_s_memtime();
                    if (TRACE && n == 0 && (abl & 128) && ((abl >> 8) & 7) == 1 && blockIdx.x == 0 && tid == 0 && t < 64) g_rnn_trace[t * 4 + 1] = __builtin_amdgcn_s_memtime();
                    if (n == NT - 1) {
                        // the next step's input terms and the row touches of the step after it, behind the LAST pull of this step: vector
                        // memory returns in order, so in front of a pull they would hold it back by their HBM latency
                        // (clamped to the last step instead of skipped: branch-free; the extra loads hit rows this launch owns)
                        retire_touch();
                        const int tn = t + 1 < T ? t + 1 : t, tn2 = t + 2 < T ? t + 2 : t;
                        request_inputs(BWD ? T - 1 - tn : tn);
                        if (!(abl & 4)) touch_rows(BWD ? T - 1 - tn2 : tn2);
                    }
                    if (NT > 1) {
                        // early request of the next pull: tile n + 1 of this step, or tile 0 of the next one
                        const int nn = (n + 1) % NT;
                        const int tq = n == NT - 1 ? t + 1 : t;              // the step that will consume it
                        // (always requested, never behind a branch: a loaded value that meets a constant at a join makes the compiler wait
                        // for it there; steps 0 and T do not pull — their request is clamped to a row of this launch and dropped)
                        const int tqc = tq < 1 ? 1 : (tq > T - 1 ? (T > 1 ? T - 1 : 1) : tq);
                        const int soq = (BWD ? T - tqc : tqc - 1) * (R * 4);
    #pragma unroll
                        for (int i = 0; i < PL; ++i) pv[i] = __builtin_amdgcn_raw_buffer_load_b128(hrs, vpull[nn] + 16 * i, soq, 16);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0, c2 = c0, c3 = c0;
                    if (t > 0 && !(abl & 2)) {
                        // A fragments in batches of AB k-blocks, NBUF batches in flight (LDS latency is 2-4 k-blocks of 4x4x1 issue time).  A batch
                        // is REQUESTED last k-block first and CONSUMED first k-block first: LDS returns in order, so the wait for the first
                        // fragment used covers the whole batch — one s_waitcnt per batch instead of one per k-block (a wave issues in order,
                        // and with a wait + a read between every four 8-cycle MFMAs it reached 73 % of the pipe's rate).  Measured (B = 256 /
                        // 1024, us): one k-block at a time 76.5 / 234; batches of 2: 75.4 / 244; of 8: 73.8 / 235.5; of 4, two in flight: 72.0-73.1 /
                        // 233 — the first MFMA of a step waits for four fragments, not eight.  The order of the sum over k is unchanged.
                        constexpr int AB = 4, NBUF = 2;
                        const float* ap = buf + n * kQ4Rows * LD + aoff;
                        float4 a[NBUF][AB];
                        auto request = [&](int b) {
    #pragma unroll
                            for (int j = AB - 1; j >= 0; --j) a[b % NBUF][j] = *reinterpret_cast<const float4*>(ap + (b * AB + j) * 16);
                        };
    #pragma unroll
                        for (int b = 0; b < NBUF; ++b) request(b);
                        __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
                        for (int b = 0; b < KB / AB; ++b) {
    #pragma unroll
                            for (int j = 0; j < AB; ++j) {
                                const float4 ak = a[b % NBUF][j];
                                const int k = b * AB + j;
                                c0 = __builtin_amdgcn_mfma_f32_4x4x1f32(ak.x, wreg[k].x, c0, 0, 0, 0);
                                c1 = __builtin_amdgcn_mfma_f32_4x4x1f32(ak.y, wreg[k].y, c1, 0, 0, 0);
                                c2 = __builtin_amdgcn_mfma_f32_4x4x1f32(ak.z, wreg[k].z, c2, 0, 0, 0);
                                c3 = __builtin_amdgcn_mfma_f32_4x4x1f32(ak.w, wreg[k].w, c3, 0, 0, 0);
                            }
                            __builtin_amdgcn_sched_barrier(0);
#ifdef TIP_MEASURE
                            // MEASUREMENT (TIP_RNN_ABLATE bit 4, wrong results): only the first NBUF batches of A fragments are read from
                            // LDS, the MFMAs of the later ones reuse their registers — 8 instead of 32 ds_read_b128 per wave and tile:
                            // what the matrix phase costs without its LDS traffic
                            if (b + NBUF < KB / AB && !(abl & 16)) request(b + NBUF);
#else
                            if (b + NBUF < KB / AB) request(b + NBUF);
#endif
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                    const f32x4 p = (c0 + c1) + (c2 + c3);   // registers = rows 0..3, one k-partial per lane group
                    // reduce-scatter over the lane groups: lane (lg, l15) ends with row lg (as tip_fused.hip's tail_reduce)
                    float a0 = p[0], a2 = p[2];
                    swap32(a0, a2);
                    float k0 = a0 + a2;
                    float a1 = p[1], a3 = p[3];
                    swap32(a1, a3);
                    float k1 = a1 + a3;
                    swap16(k0, k1);
                    const float acc = k0 + k1;
                    if (TRACE && !(abl & 128) && n == 0 && blockIdx.x == 0 && tid == 0 && t < 64) {
                        asm volatile("" :: "v"(acc));
                        g_rnn_trace[t * 4 + 1] = __builtin_amdgcn_s_memtime();
                    }
                    if (TRACE && (abl & 128) && ((abl >> 8) & 7) == 2 && n == 0 && blockIdx.x == 0 && tid == 0 && t < 64) {
                        asm volatile("" :: "v"(c0[0]), "v"(c1[0]), "v"(c2[0]), "v"(c3[0]));   // MFMAs of tile 0 done, before the reduction
                        g_rnn_trace[t * 4 + 1] = __builtin_amdgcn_s_memtime();
                    }
#ifdef TIP_MEASURE
                    // MEASUREMENT (TIP_RNN_ABLATE bit 5, wrong results): a clamp instead of tanh (exp + IEEE division, ~25 dependent
                    // vector instructions between the last MFMA and the state store): what the activation costs on the serial chain
                    float hv = BWD ? (acc + ihv[n]) * (1.0f - gv[n] * gv[n])
                                   : ((abl & 32) ? fminf(fmaxf(acc + ihv[n], -1.0f), 1.0f) : tip_tanh(acc + ihv[n]));
#else
                    float hv = BWD ? (acc + ihv[n]) * (1.0f - gv[n] * gv[n]) : tip_tanh(acc + ihv[n]);
#endif
                    if (hv != hv) hv = __uint_as_float(kPoisonBits);   // poison travels as the canonical NaN, never as the sentinel
                    // same XCD (verified): a plain store lands in the shared L2 (L1 is write-through); otherwise sc1 = write-through
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hv), hrs, vout[n], so_out, SAME_XCD ? 0 : 16);
                }
                if (TRACE && blockIdx.x == 0 && tid == 0 && t < 64) g_rnn_trace[t * 4 + 2] = __builtin_amdgcn_s_memtime();
            }
            retire_touch();
            __syncthreads();   // the next batch's second step rewrites the buffer the last step of this one may still be reading
        }
    };
    if (same_xcd) run_steps(std::true_type{});
    else run_steps(std::false_type{});
    // leave the XCC-exchange word cleared for a replay of this launch from a HIP graph (same tag): see rnn_resident_kernel
    if (T >= 2 && tid == 0 && !dead) __hip_atomic_store(flags + group * CLUSTER + cid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
