    using namespace fz;
    using namespace fzh;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X = smem;
    float* C = smem + X_FLOATS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wts), 0, wbytes, 0x00020000);
    const int voff = lane * 16;
    // this lane's LDS offsets (floats) inside a [rows][ld] operand: 16-row blocks / tail blocks
    auto am = [&](int ld) { return l15 * ld + lg * 4; };
    auto at = [&](int ld) { return (TAIL0 + (lane & 3)) * ld + lg * 4; };
    // LIVE: the deployed forward (tip_forward_live) — the TR instantiation's four dropout sites and the past-state keep mask drawn in the
    // prologue, no stash; the inference instantiation's outputs.  Both seeds come from lv.seeds (device, {seed, state_seed}) when given:
    // scalar loads, and every key below is computed from them once per site on the scalar unit.
    constexpr bool DR = TR || LIVE;
    const LiveArgs lv = live_args_of(tr);
    unsigned long long dseed = tr.seed, sseed = 0;
    if (LIVE) {
        sseed = lv.state_seed;
        if (lv.seeds) { dseed = lv.seeds[0]; sseed = lv.seeds[1]; }
    }
    const unsigned mkey = LIVE && lv.mthresh ? tip_drop_key_s(sseed, kStateMaskSite) : 0u;

    // rows 40..47 of the residual stream: zero once, never written again (finite pad keys / values for the attention)
    for (int i = tid; i < 8 * LDX; i += THREADS) X[TMAX * LDX + i] = 0.f;

    for (int win = ctl.first(); win < B; win += ctl.stride()) {
        WRing<3> g_qkv;
        {
        const int layer = -1;
        FH_STAMP(0);
        if (TRACE && tid == 0 && win == (int)blockIdx.x && blockIdx.x < 1024) g_fh_wg[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        const int in_soff = (int)(IN_W * 4) + (wave * 2) * (KIN / 16) * 1024;
        WRing<2> g_in;
        ring_prefetch<2>(g_in, rsrc, voff, in_soff, (KIN / 16) * 1024);
        // ---- P0 prologue (:63-78) ------------------------------------------------------------------------------------
        float* U = C;
        for (int i = tid; i < RP * LDU / 4; i += THREADS) reinterpret_cast<float4*>(U)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        {
            // Round 3: rows wave, wave + 8, ... (five per wave at T = 40), a lane per column: unit-stride loads without an index
            // division, ALL of a wave's loads in flight before the first is used, unconditional (clamped addresses), and the LDS
            // stores through one base + COMPILE-TIME offsets.  The element loop this replaces (i = tid, tid + 512, ...: 18 trips,
            // each a dependent HBM round trip behind an integer division) took 17.2 k cycles per window; a first attempt at
            // batching the loads (round 2) spilled its forty store addresses and was slower.
            constexpr int NR = (TMAX + 7) / 8;
            float vi[NR][2], vs[NR][3], vk[NR][3];
            const float* kmb = keep_mask ? keep_mask : x_s;
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const int r = wave + 8 * j;
                const int rc = r < T ? r : T - 1;
                const float* xi = x_imu + ((size_t)win * T + rc) * NI;
                const float* xs = x_s + ((size_t)win * T + rc) * S;
                const float* km = kmb + ((size_t)win * T + rc) * S;
#pragma unroll
                for (int q = 0; q < 2; ++q) vi[j][q] = xi[lane + 64 * q < NI ? lane + 64 * q : NI - 1];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int c = lane + 64 * q < S ? lane + 64 * q : S - 1;
                    vs[j][q] = xs[c];
                    vk[j][q] = km[c];
                }
            }
            float* pu_i = U + wave * LDU + lane;
            float* pu_s = pu_i + NI;
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                if (wave + 8 * j < T) {
#pragma unroll
                    for (int q = 0; q < 2; ++q)
                        if (lane + 64 * q < NI) pu_i[8 * j * LDU + 64 * q] = vi[j][q];
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        if (lane + 64 * q < S) {
                            float v = vs[j][q];
                            if (v != v) v = 0.f;                               // :65
                            if (keep_mask) v = v * vk[j][q] * keep_scale;     // :77 with an explicit keep-mask
                            else if (LIVE && lv.mthresh)                       // ... or drawn here: tip_draw_keep_mask's decision of this element of x_s
                                v = v * (tip_drop_hash_k(mkey, ((unsigned)win * (unsigned)T + (unsigned)(wave + 8 * j)) * (unsigned)S + (unsigned)(lane + 64 * q)) >= lv.mthresh ? 1.f : 0.f) * keep_scale;
                            pu_s[8 * j * LDU + 64 * q] = v;
                        }
                }
            }
        }
        __syncthreads();
        FH_STAMP(1);
        // training forward: the staged input rows are dW_in's operand in the backward — stashed from here instead of by a launch of
        // their own (tip_train.hip)
        if (TR && tr.u) rows_to_hbm_fixed<KIN>(U, LDU, tr.sv + (size_t)tr.u * 64 + (size_t)win * T * KIN, KIN, T, opaque(tid));
        // ---- P1 in_linear (:79) + channel shuffle (folded) -------------------------------------------------------------
        {
            f32x4 acc[RBM][2], acct[RBT][2];
            zero_acc_h<2>(acc, acct);
            gemm_phase_h<2, KIN / 16, 0, TR>(acc, acct, U + am(LDU), U + at(LDU), LDU, rsrc, voff, in_soff, (KIN / 16) * 1024, g_in, in_soff,
                                      (KIN / 16) * 1024);
            ring_prefetch<3>(g_qkv, rsrc, voff, (int)(LAYER0 * 4) + (int)(QKV_W * 4) + wave * 16 * 1024, 16 * 16 * 1024);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int col = (wave * 2 + n) * 16 + l15;
                const float bv = wts[IN_B + col];
#pragma unroll
                for (int r = 0; r < RBM; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) X[(r * 16 + lg * 4 + e) * LDX + col] = acc[r][n][e] + bv;
#pragma unroll
                for (int r = 0; r < RBT; ++r) X[(TAIL0 + 4 * r + lg) * LDX + col] = tail_reduce(acct[r][n], lg) + bv;
            }
        }
        __syncthreads();
        FH_STAMP(2);
        }
        const size_t grow0 = (size_t)win * T;           // first global row (b*T + t) of this window
        if (TR) rows_to_hbm_fixed<D>(X, LDX, tr.sv + (size_t)tr.x0 * 64 + grow0 * D, D, T, opaque(tid));
#pragma unroll 1
        for (int layer = 0; layer < L; ++layer) {
            FH_STAMP(8);
            const float* LW = wts + LAYER0 + (size_t)layer * LAYER_FLOATS;
            const int lbase = (int)((LAYER0 + (size_t)layer * LAYER_FLOATS) * 4);
            float* svl = TR ? tr.sv + (size_t)layer * tr.layer_stride * 64 : nullptr;   // this layer's stash
            const unsigned dk1 = DR ? tip_drop_key_s(dseed, (unsigned)(layer * 4 + 1)) : 0u;
            const unsigned dk2 = DR ? tip_drop_key_s(dseed, (unsigned)(layer * 4 + 2)) : 0u;
            const unsigned dk3 = DR ? tip_drop_key_s(dseed, (unsigned)(layer * 4 + 3)) : 0u;
            float bvo[2], bv2[2];   // out-projection / linear2 biases of this wave's columns: requested a phase (or eight) ahead of their use
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                bvo[n] = LW[WO_B + (wave * 2 + n) * 16 + l15];
                bv2[n] = LW[W2_B + (wave * 2 + n) * 16 + l15];
            }
            WRing<2> g_o, g_f;
            // ---- self-attention block.  Wave w owns heads w and 8 + w END TO END and runs them back to back with no workgroup
            // barrier in between: projection -> attention -> projection -> attention.  The two waves that share a SIMD drift apart
            // in this stretch, so one's softmax (VALU, LDS) runs under the other's projection MFMAs instead of both idling the
            // matrix pipe at the same time in front of a barrier; then ONE out-projection over all 16 heads (K = 256).
            float* Oc = C;   // attention output of all heads [48 rows][256 channels], leading dimension LDX: the out-projection's A operand
#pragma unroll 1
            for (int c = 0; c < 2; ++c) {
                const int head = c * 8 + wave;
                f32x4 acc[RBM][3], acct[RBT][3];
                zero_acc_h<3>(acc, acct);
                const int qsoff = lbase + (int)(QKV_W * 4) + head * 16 * 1024;
                // rows 0..31: Q and K with swapped operands (their accumulators are the attention's transposed fragments), V plain;
                // rows 32..39: all three through the 4x4x1 tail in the plain orientation.  The tail of head w's product primes
                // the ring with head 8 + w's first fragments (they fly during head w's attention).
                const int nxt = c == 0 ? qsoff + 8 * 16 * 1024 : qsoff;
                gemm_phase_h<3, 16, 2, TR>(acc, acct, X + am(LDX), X + at(LDX), LDX, rsrc, voff, qsoff, 16 * 16 * 1024, g_qkv, nxt,
                                       16 * 16 * 1024);
                if (c == 1)   // out-projection fragments fly during the second attention and the barrier
                    ring_prefetch<2>(g_o, rsrc, voff, lbase + (int)(WO_W * 4) + (wave * 2) * 16 * 1024, 16 * 1024);
                const f32x4 bq = *reinterpret_cast<const f32x4*>(LW + QKV_B + head * 16 + lg * 4);
                const f32x4 bk = *reinterpret_cast<const f32x4*>(LW + QKV_B + D + head * 16 + lg * 4);
                const float bv = LW[QKV_B + 2 * D + head * 16 + l15];
                f32x4 qt[RB], kt[RB], vv[RB];
#pragma unroll
                for (int r = 0; r < RBM; ++r) {
                    qt[r] = acc[r][0] + bq;
                    kt[r] = acc[r][1] + bk;
                    vv[r] = acc[r][2] + bv;
                }
                // Third row block (rows 32..47, eight of them real).  V: gather the tail into the plain layout.  Q, K: the tail
                // yields (row 4 rb + lg, channel l15) per lane; the attention wants (row l15, channels 4 lg ..): a 1.3-KB per-wave
                // LDS patch behind the O plane does the transpose, no workgroup barrier — a wave's LDS operations complete in
                // program order.
                vv[2] = tail_gather_v(acct[0][2], acct[1][2], lg);
                if (lg < 2) vv[2] += bv;
                {
                    constexpr int SLD = 20;                                   // 16 channels + 4: b128 reads of 8 rows conflict-free
                    float* scr = C + RP * LDX + wave * (2 * 8 * SLD);
                    const float bqp = LW[QKV_B + head * 16 + l15], bkp = LW[QKV_B + D + head * 16 + l15];
#pragma unroll
                    for (int rb = 0; rb < RBT; ++rb) {
                        scr[(4 * rb + lg) * SLD + l15] = tail_reduce(acct[rb][0], lg) + bqp;
                        scr[8 * SLD + (4 * rb + lg) * SLD + l15] = tail_reduce(acct[rb][1], lg) + bkp;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                    qt[2] = l15 < 8 ? *reinterpret_cast<const f32x4*>(scr + l15 * SLD + lg * 4) : z;
                    kt[2] = l15 < 8 ? *reinterpret_cast<const f32x4*>(scr + 8 * SLD + l15 * SLD + lg * 4) : z;
                    __builtin_amdgcn_wave_barrier();                          // (the patch is rewritten by this wave's next head)
                }
                FH_STAMP(9 + 4 * c);    // QKV projection issued and its results consumed
                if (TR) {
                    // raw q (the packed W_q carries the 1/sqrt(d_head) fold: undo it exactly), k, v -> [M, 3D]; the third block has
                    // the same fragment layout as the padded kernel's (rows 32 + l15 / rows 32 + 4 lg + e), pad rows masked by T
                    // (a buffer of this window's T rows: the pad rows' stores are dropped by the range check, not by a branch each)
                    const __amdgpu_buffer_rsrc_t qp_rs = tip_rows_buffer(svl + (size_t)tr.qkv * 64 + grow0 * (3 * D), T * 3 * D * 4);
                    const int lo = opaque(lane), l15o = lo & 15, lgo = lo >> 4;
#pragma unroll
                    for (int r = 0; r < RB; ++r) {
                        const int qo = ((r * 16 + l15o) * (3 * D) + head * 16 + lgo * 4) * 4;
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, qt[r] * 4.0f), qp_rs, qo, 0, kTipNT);
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, kt[r]), qp_rs, qo + D * 4, 0, kTipNT);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vv[r][e]), qp_rs,
                                                                  ((r * 16 + lgo * 4 + e) * (3 * D) + 2 * D + head * 16 + l15o) * 4, 0, kTipNT);
                    }
                    attention_head_regs<LDX, true>(qt, kt, vv, Oc, head * 16, lo, TMAX, svl + (size_t)tr.ast * 64,
                                                   (unsigned long long)win * H + head, T, tr.seed, (unsigned)(layer * 4 + 0), tr.thresh,
                                                   tr.scale);
                } else if (LIVE) {   // dropout on the probabilities as TR draws it, no statistics
                    attention_head_regs<LDX, true, false>(qt, kt, vv, Oc, head * 16, opaque(lane), TMAX, nullptr, (unsigned long long)win * H + head, T,
                                                          dseed, (unsigned)(layer * 4 + 0), tr.thresh, tr.scale);
                } else {
                    attention_head_regs<LDX>(qt, kt, vv, Oc, head * 16, lane, TMAX);   // rows 40..47 of the O plane are never read
                }
                FH_STAMP(10 + 4 * c);
            }
            __syncthreads();
            FH_STAMP(15);
            if (TR) rows_to_hbm_fixed<D>(Oc, LDX, svl + (size_t)tr.att * 64 + grow0 * D, D, T, opaque(tid));
            ring_prefetch<2>(g_f, rsrc, voff, lbase + (int)(W1_W * 4) + (wave * 2) * 16 * 1024, 16 * 1024);
            f32x4 acc_o[RBM][2], acc_ot[RBT][2];
            zero_acc_h<2>(acc_o, acc_ot);
            {
                const int osoff = lbase + (int)(WO_W * 4) + (wave * 2) * 16 * 1024;
                gemm_phase_h<2, 16, 0, TR>(acc_o, acc_ot, Oc + am(LDX), Oc + at(LDX), LDX, rsrc, voff, osoff, 16 * 1024, g_o, osoff, 16 * 1024);
            }
            __syncthreads();
            FH_STAMP(16);
            // residual + bias, then LayerNorm1.  The residual values of this lane's 20 elements are READ before the first is written
            // back: `X[i] += v` per element compiles to a chain of ds_read -> wait -> ds_write round trips (2-3 k cycles per epilogue
            // with the matrix pipe idle; the optimiser may not move a read across a write it cannot prove disjoint).
            float xr[2][RBM][4], xt[2][RBT];
#pragma unroll
            for (int n = 0; n < 2; ++n) {   // (the unroll pragma above binds to this loop)
                const int col = (wave * 2 + n) * 16 + l15;
#pragma unroll
                for (int r = 0; r < RBM; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) xr[n][r][e] = X[(r * 16 + lg * 4 + e) * LDX + col];
#pragma unroll
                for (int r = 0; r < RBT; ++r) xt[n][r] = X[(TAIL0 + 4 * r + lg) * LDX + col];
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int col = (wave * 2 + n) * 16 + l15;
                const float bv = bvo[n];
                    const int hl = LIVE ? opaque(lane) : lane, hlg = LIVE ? hl >> 4 : lg, hcol = LIVE ? (wave * 2 + n) * 16 + (hl & 15) : col;   // (LIVE: the hash indices are formed here, not hoisted out of the layer loop and spilled)
#pragma unroll
                for (int r = 0; r < RBM; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v = acc_o[r][n][e] + bv;
                        if (DR && tr.thresh)
                            v = tip_drop_hash_k(dk1, (grow0 + r * 16 + hlg * 4 + e) * D + hcol) >= tr.thresh ? v * tr.scale : 0.f;
                        X[(r * 16 + lg * 4 + e) * LDX + col] = xr[n][r][e] + v;
                    }
#pragma unroll
                for (int r = 0; r < RBT; ++r) {
                    float v = tail_reduce(acc_ot[r][n], lg) + bv;
                    if (DR && tr.thresh)
                        v = tip_drop_hash_k(dk1, (grow0 + TAIL0 + 4 * r + hlg) * D + hcol) >= tr.thresh ? v * tr.scale : 0.f;
                    X[(TAIL0 + 4 * r + lg) * LDX + col] = xt[n][r] + v;
                }
            }
            __syncthreads();
            FH_STAMP(17);
            if (TR)
                layernorm_rows16<fz::TMAX, fz::LDX, true>(X, LW + G1, LW + BE1, wave, opaque(lane), svl + (size_t)tr.z1 * 64 + grow0 * D,
                                                          svl + (size_t)tr.st1 * 64 + grow0 * 2, svl + (size_t)tr.x1 * 64 + grow0 * D, T);
            else
                layernorm_rows16<fz::TMAX, fz::LDX>(X, LW + G1, LW + BE1, wave, lane);   // rows 40..47 stay zero
            __syncthreads();
            FH_STAMP(18);
            // ---- feed-forward block: hidden in 4 chunks of 256, linear2 accumulates in registers -------------------------
            float* Hc = C;
            f32x4 acc_f[RBM][2], acc_ft[RBT][2];
            zero_acc_h<2>(acc_f, acc_ft);
#pragma unroll 1
            for (int f = 0; f < 4; ++f) {
                {
                    f32x4 acc[RBM][2], acct[RBT][2];
                    zero_acc_h<2>(acc, acct);
                    const int nb0 = f * 16 + wave * 2;
                    const int w1off = lbase + (int)(W1_W * 4) + nb0 * 16 * 1024;
                    const int w2off = lbase + (int)(W2_W * 4) + ((wave * 2) * 64 + f * 16) * 1024;
                    // (the epilogue's bias is requested BEFORE the product: after it, the L2 round trip would be exposed 16 times a layer)
                    float bv1[2];
#pragma unroll
                    for (int n = 0; n < 2; ++n) bv1[n] = LW[W1_B + f * 256 + (wave * 2 + n) * 16 + l15];
                    gemm_phase_h<2, 16, 0, TR>(acc, acct, X + am(LDX), X + at(LDX), LDX, rsrc, voff, w1off, 16 * 1024, g_f, w2off, 64 * 1024);
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const int col = (wave * 2 + n) * 16 + l15;
                        const float bv = bv1[n];
                    const int hl = LIVE ? opaque(lane) : lane, hlg = LIVE ? hl >> 4 : lg, hcol = LIVE ? (wave * 2 + n) * 16 + (hl & 15) : col;   // (LIVE: the hash indices are formed here, not hoisted out of the layer loop and spilled)
#pragma unroll
                        for (int r = 0; r < RBM; ++r)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                float v = fmaxf(acc[r][n][e] + bv, 0.f);
                                if (DR && tr.thresh)
                                    v = tip_drop_hash_k(dk2, (grow0 + r * 16 + hlg * 4 + e) * F + f * 256 + hcol) >= tr.thresh ? v * tr.scale : 0.f;
                                Hc[(r * 16 + lg * 4 + e) * LDX + col] = v;
                            }
#pragma unroll
                        for (int r = 0; r < RBT; ++r) {
                            float v = fmaxf(tail_reduce(acct[r][n], lg) + bv, 0.f);
                            if (DR && tr.thresh)
                                v = tip_drop_hash_k(dk2, (grow0 + TAIL0 + 4 * r + hlg) * F + f * 256 + hcol) >= tr.thresh ? v * tr.scale : 0.f;
                            Hc[(TAIL0 + 4 * r + lg) * LDX + col] = v;
                        }
                    }
                }
                FH_STAMP(19 + 3 * f);
                __syncthreads();
                FH_STAMP(20 + 3 * f);
                if (TR)   // (the gate bits sit behind the layer's [M][F] hidden rows: saved_layout, tip_train.hip)
                    hidden_to_hbm(Hc, LDX, svl + (size_t)tr.hid * 64 + grow0 * F + f * 256, F,
                                  reinterpret_cast<unsigned*>(svl + (size_t)tr.hid * 64 + (size_t)B * T * F) + grow0 * 32, f, T, opaque(tid));
                {
                    const int w2off = lbase + (int)(W2_W * 4) + ((wave * 2) * 64 + f * 16) * 1024;
                    const int nxt = f < 3 ? lbase + (int)(W1_W * 4) + ((f + 1) * 16 + wave * 2) * 16 * 1024 : w2off;
                    gemm_phase_h<2, 16, 0, TR>(acc_f, acc_ft, Hc + am(LDX), Hc + at(LDX), LDX, rsrc, voff, w2off, 64 * 1024, g_f, nxt,
                                        f < 3 ? 16 * 1024 : 64 * 1024);
                }
                __syncthreads();
                FH_STAMP(21 + 3 * f);
            }
            if (layer + 1 < L)
                ring_prefetch<3>(g_qkv, rsrc, voff, lbase + (int)(LAYER_FLOATS * 4) + (int)(QKV_W * 4) + wave * 16 * 1024, 16 * 16 * 1024);
#pragma unroll
            for (int n = 0; n < 2; ++n) {   // residual values first (as after the out-projection)
                const int col = (wave * 2 + n) * 16 + l15;
#pragma unroll
                for (int r = 0; r < RBM; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) xr[n][r][e] = X[(r * 16 + lg * 4 + e) * LDX + col];
#pragma unroll
                for (int r = 0; r < RBT; ++r) xt[n][r] = X[(TAIL0 + 4 * r + lg) * LDX + col];
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int col = (wave * 2 + n) * 16 + l15;
                const float bv = bv2[n];
                    const int hl = LIVE ? opaque(lane) : lane, hlg = LIVE ? hl >> 4 : lg, hcol = LIVE ? (wave * 2 + n) * 16 + (hl & 15) : col;   // (LIVE: the hash indices are formed here, not hoisted out of the layer loop and spilled)
#pragma unroll
                for (int r = 0; r < RBM; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v = acc_f[r][n][e] + bv;
                        if (DR && tr.thresh)
                            v = tip_drop_hash_k(dk3, (grow0 + r * 16 + hlg * 4 + e) * D + hcol) >= tr.thresh ? v * tr.scale : 0.f;
                        X[(r * 16 + lg * 4 + e) * LDX + col] = xr[n][r][e] + v;
                    }
#pragma unroll
                for (int r = 0; r < RBT; ++r) {
                    float v = tail_reduce(acc_ft[r][n], lg) + bv;
                    if (DR && tr.thresh)
                        v = tip_drop_hash_k(dk3, (grow0 + TAIL0 + 4 * r + hlg) * D + hcol) >= tr.thresh ? v * tr.scale : 0.f;
                    X[(TAIL0 + 4 * r + lg) * LDX + col] = xt[n][r] + v;
                }
            }
            __syncthreads();
            FH_STAMP(31);
            if (TR)
                layernorm_rows16<fz::TMAX, fz::LDX, true>(X, LW + G2, LW + BE2, wave, opaque(lane), svl + (size_t)tr.z2 * 64 + grow0 * D,
                                                          svl + (size_t)tr.st2 * 64 + grow0 * 2, svl + (size_t)tr.xo * 64 + grow0 * D, T);
            else
                layernorm_rows16<fz::TMAX, fz::LDX>(X, LW + G2, LW + BE2, wave, lane);
            __syncthreads();
            FH_STAMP(32);
        }
        { const int layer = -1; FH_STAMP(40); }
        // ---- RNN input projection: IH = X W_ih^T + (b_ih + b_hh), rows 0..T-1 -> HBM -------------------------------------
        if (ih_out) {
            f32x4 acc[RBM][4], acct[RBT][4];
            zero_acc_h<4>(acc, acct);
            const int isoff = ih_off_b + (wave * 4) * 16 * 1024;
            WRing<4> g_ih;
            ring_prefetch<4>(g_ih, rsrc, voff, isoff, 16 * 1024);
            // Round 3: the 16-row blocks with SWAPPED operands — transposed accumulators, (columns 16 n + 4 lg + e, row 16 r + l15): a
            // lane stores four consecutive columns of one row with ONE 16-byte store instead of four scattered 4-byte ones (the
            // store tail is issue-bound: 32 -> 8 store instructions per wave for rows 0-31).  Same products, same sums.
            gemm_phase_h<4, 16, 4, TR>(acc, acct, X + am(LDX), X + at(LDX), LDX, rsrc, voff, isoff, 16 * 1024, g_ih, isoff, 16 * 1024);
            // This window's IH rows as a buffer of T rows: the stores of the pad rows are dropped by the range check, not by a branch
            // around each store.  The biases of all four column blocks are requested BEFORE the first store: loaded inside the loop, each
            // block's bias load sat behind the previous block's stores (the optimiser may not hoist a load over a store it cannot prove
            // disjoint) — four exposed L2 round trips at the end of every window.
            const __amdgpu_buffer_rsrc_t io_rs = __builtin_amdgcn_make_buffer_rsrc(ih_out + (size_t)win * T * R, 0, T * R * 4, 0x00020000);
            // (opaque lane index: the store offsets are formed here, not hoisted to the top of the kernel and carried in scratch)
            const int lo = opaque(lane), l15o = lo & 15, lgo = lo >> 4;
            float bvs[4];
            f32x4 bv4s[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                bvs[n] = wts[ih_off_b / 4 + R * D + (wave * 4 + n) * 16 + l15o];
                bv4s[n] = *reinterpret_cast<const f32x4*>(wts + ih_off_b / 4 + R * D + (wave * 4 + n) * 16 + lgo * 4);
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = (wave * 4 + n) * 16 + l15o;
#pragma unroll
                for (int r = 0; r < RBM; ++r) {
                    const int row = r * 16 + l15o;
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[r][n] + bv4s[n]), io_rs, (row * R + (wave * 4 + n) * 16 + lgo * 4) * 4, 0, Ctl::kAux);
                }
#pragma unroll
                for (int r = 0; r < RBT; ++r) {
                    const float v = tail_reduce(acct[r][n], lg) + bvs[n];
                    const int row = TAIL0 + 4 * r + lgo;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), io_rs, (row * R + col) * 4, 0, Ctl::kAux);
                }
            }
        }
        if (hall_sentinel) {
            if constexpr (Ctl::kAux != 0) {   // the same words through the write-through store form
                const __amdgpu_buffer_rsrc_t hs_rs = __builtin_amdgcn_make_buffer_rsrc(hall_sentinel + (size_t)win * T * R, 0, T * R * 4, 0x00020000);
                const u32x4 ones = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
                for (int i = opaque(tid); i < T * (R / 4); i += THREADS) __builtin_amdgcn_raw_buffer_store_b128(ones, hs_rs, i * 16, 0, Ctl::kAux);
            } else {
            uint4* hp = reinterpret_cast<uint4*>(hall_sentinel + (size_t)win * T * R);
            for (int i = opaque(tid); i < T * (R / 4); i += THREADS) hp[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            }
        }
        if (xout) {
            float* out = xout + (size_t)win * T * D;
            for (int i = tid; i < T * (D / 4); i += THREADS) {
                const int r = i / (D / 4), c4 = i - r * (D / 4);
                *reinterpret_cast<float4*>(out + (size_t)r * D + c4 * 4) = *reinterpret_cast<const float4*>(X + r * LDX + c4 * 4);
            }
        }
        __syncthreads();
        { const int layer = -1; FH_STAMP(41); }
        if (TRACE && tid == 0 && blockIdx.x < 1024) g_fh_wg[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
        ctl.published(win, tid);
    }
