// tip_fused.hip — fused execution plan for the paper configuration (d=256, 16 heads x 16, ffn=1024, T<=40).
//
// One 512-thread workgroup (8 waves, 2 per SIMD) carries ONE 40-frame window through the prologue, in_linear
// and all encoder layers without leaving the CU: the activations [48 x 256] live in LDS for the whole pass,
// every GEMM is v_mfma_f32_16x16x4_f32 with the A operand read from LDS (ds_read_b128 = 4 k-steps) and the B
// operand streamed straight from L2 in pre-packed fragment order (one coalesced 1-KiB global_load_dwordx4 per
// 16x16 weight block per wave, register double-buffered), attention runs one head per wave between the QKV
// GEMM and the out-projection with no inter-wave dependency, LayerNorm uses wave shuffles.  HBM sees only the
// window's inputs (35 KB) and the encoder output (40 KB); weights (12.6 MB) are L2/Infinity-Cache resident and
// shared by all 256 CUs.  Reference: /root/reference/simple_transformer_with_state.py:63-91.
//
// LDS map (floats):  X [48][260] residual stream | C chunk region: Q [48][132] | K [48][132] | V^T [128][52] of 8
//                    heads, reused as U [48][228] (prologue) and Hc [48][260] (FFN hidden chunk).  127,232 B.
#include <stdlib.h>
#include <string.h>

#include "tip_fused_h.h"   // namespace fz, the device pieces, the hybrid encoder's body

namespace tip {

bool fused_supported(const Dims& d, int T) {
    return d.D == fz::D && d.H == fz::H && d.F == fz::F && d.In <= fz::KIN && T >= 1 && T <= fz::TMAX && d.L >= 1;
}

// RNN input projection (R = 512) rides at the end of the fused section: [32 nb][16 kb] fragments + (b_ih + b_hh)
bool fused_has_rnn_ih(const Dims& d) { return d.with_rnn && d.R == fz::R; }
static size_t fused_ih_off(const Dims& d) { return fz::LAYER0 + (size_t)d.L * fz::LAYER_FLOATS; }

size_t fused_packed_floats(const Dims& d) {
    if (!(d.D == fz::D && d.H == fz::H && d.F == fz::F && d.In <= fz::KIN)) return 0;
    return fused_ih_off(d) + (fused_has_rnn_ih(d) ? (size_t)fz::R * fz::D + fz::R : 0) + fz::TAIL_PAD;
}

// The fused section of the image: weights in 16x16x4 B-fragment order [N/16][Kpad/16][64 lanes][4],
//   dst[((nb*KB + kb)*64 + lane)*4 + s] = W[nb*16 + (lane&15)][kb*16 + 4*(lane>>4) + s],
// with the folds: channel shuffle (:88-89) into in_linear's rows, root-velocity columns (:75) zeroed, 1/sqrt(16) into W_q (exact)
void fused_pack_ops(const Dims& d, const float* const* t, size_t base, std::vector<PackOp>& ops) {
    using namespace fz;
    auto frag = [](const float* W, size_t dst, int N, int K) { return frag_op(W, dst, N, K, N, K); };
    auto vec = [](const float* v, size_t dst, int N) { return rows_op(v, dst, N, 1, N, 1); };
    {
        PackOp o = frag_op(t[0], base + IN_W, D, KIN, D, d.In);
        o.shuffle_h = H; o.shuffle_dh = DH;
        o.z0 = d.n_imu_total + d.rootv0; o.z1 = d.n_imu_total + d.rootv1;
        ops.push_back(o);
        PackOp b = vec(t[1], base + IN_B, D);
        b.shuffle_h = H; b.shuffle_dh = DH;
        ops.push_back(b);
    }
    for (int l = 0; l < d.L; ++l) {
        const float* const* lw = t + 2 + 12 * l;
        const size_t L = base + LAYER0 + (size_t)l * LAYER_FLOATS;
        PackOp q = frag(lw[0], L + QKV_W, 3 * D, D);
        q.scale = 0.25f; q.scale_rows = D;
        ops.push_back(q);
        PackOp qb = vec(lw[1], L + QKV_B, 3 * D);
        qb.scale = 0.25f; qb.scale_rows = D;
        ops.push_back(qb);
        ops.push_back(frag(lw[2], L + WO_W, D, D));
        ops.push_back(vec(lw[3], L + WO_B, D));
        ops.push_back(frag(lw[4], L + W1_W, F, D));
        ops.push_back(vec(lw[5], L + W1_B, F));
        ops.push_back(frag(lw[6], L + W2_W, D, F));
        ops.push_back(vec(lw[7], L + W2_B, D));
        ops.push_back(vec(lw[8], L + G1, D));
        ops.push_back(vec(lw[9], L + BE1, D));
        ops.push_back(vec(lw[10], L + G2, D));
        ops.push_back(vec(lw[11], L + BE2, D));
    }
    if (fused_has_rnn_ih(d)) {
        const float* const* tw = t + 2 + 12 * d.L;
        const size_t I = base + fused_ih_off(d);
        ops.push_back(frag(tw[0], I, R, D));
        PackOp b = vec(tw[2], I + (size_t)R * D, R);
        b.src2 = tw[3];
        ops.push_back(b);
    }
}


// TIP_PLAN_FUSED: the 48-row inference kernel.  (The training, live and traced forwards are fused_encoder_h_kernel's.)
// The last argument is not read.  It holds the place of the hybrid kernel's FusedTrain in the kernel-argument block: the implicit
// arguments (gridDim) sit behind it, and their offset is a constant in the code, which is the code the plan's tests and figures are of.
__global__ __launch_bounds__(fz::THREADS) void fused_encoder_kernel(
    const float* __restrict__ wts, const float* __restrict__ x_imu, const float* __restrict__ x_s,
    const float* __restrict__ keep_mask, float keep_scale, float* __restrict__ xout, float* __restrict__ ih_out,
    unsigned* __restrict__ hall_sentinel, int B, int T, int NI, int S, int L, int wbytes, int ih_off_b, FusedTrain) {
    using namespace fz;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X = smem;
    float* C = smem + X_FLOATS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wts), 0, wbytes, 0x00020000);
    const int voff = lane * 16;

    for (int win = blockIdx.x; win < B; win += gridDim.x) {
        // weight fragments of the first GEMM are requested before the window's inputs are even staged
        const int in_soff = (int)(IN_W * 4) + (wave * 2) * (KIN / 16) * 1024;
        WRing<2> g_in;
        ring_prefetch<2>(g_in, rsrc, voff, in_soff, (KIN / 16) * 1024);
        WRing<3> g_qkv;   // primed one phase ahead of every QKV projection
        // ---- P0 prologue (:63-78): U = [x_imu | scrub(x_s) * mask | 0], rows >= T zero ---------------------------
        float* U = C;
        for (int i = tid; i < RP * LDU; i += THREADS) U[i] = 0.f;
        __syncthreads();
        {
            const float* xi = x_imu + (size_t)win * T * NI;
            for (int i = tid; i < T * NI; i += THREADS) {
                const int r = i / NI, c = i - r * NI;
                U[r * LDU + c] = xi[i];
            }
            const float* xs = x_s + (size_t)win * T * S;
            const float* km = keep_mask ? keep_mask + (size_t)win * T * S : nullptr;
            for (int i = tid; i < T * S; i += THREADS) {
                const int r = i / S, c = i - r * S;
                float v = xs[i];
                if (v != v) v = 0.f;                  // :65
                if (km) v = v * km[i] * keep_scale;   // :77 with an explicit keep-mask
                U[r * LDU + NI + c] = v;
            }
        }
        __syncthreads();
        // ---- P1 in_linear (:79) + channel shuffle (:88-89, folded into the packed rows) ---------------------------
        {
            f32x4 acc[RB][2];
            zero_acc<2>(acc);
            gemm_phase<2, KIN / 16, 0, false>(acc, U + l15 * LDU + lg * 4, LDU, rsrc, voff, in_soff, (KIN / 16) * 1024, g_in, in_soff,
                                    (KIN / 16) * 1024);
            // layer 0, chunk 0 QKV fragments fly during the epilogue + barrier
            ring_prefetch<3>(g_qkv, rsrc, voff, (int)(LAYER0 * 4) + (int)(QKV_W * 4) + wave * 16 * 1024, 16 * 16 * 1024);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int col = (wave * 2 + n) * 16 + l15;
                const float bv = wts[IN_B + col];
#pragma unroll
                for (int r = 0; r < RB; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) X[(r * 16 + lg * 4 + e) * LDX + col] = acc[r][n][e] + bv;
            }
        }
        __syncthreads();

#pragma unroll 1
        for (int layer = 0; layer < L; ++layer) {
            const float* LW = wts + LAYER0 + (size_t)layer * LAYER_FLOATS;
            const int lbase = (int)((LAYER0 + (size_t)layer * LAYER_FLOATS) * 4);
            float* Qc = C;   // attention output of one 8-head chunk [48 rows][128 channels]: the out-projection's A operand
            // ---- self-attention block: two chunks of 8 heads; wave w owns head 8c + w end to end -----------------
            f32x4 acc_o[RB][2];
            zero_acc<2>(acc_o);
            WRing<2> g_o, g_f;

#pragma unroll 1
            for (int c = 0; c < 2; ++c) {
                {
                    const int head = c * 8 + wave;
                    f32x4 acc[RB][3];
                    zero_acc<3>(acc);
                    // column blocks of this head in the packed [48 nb][16 kb] QKV matrix: Q = head, K = 16+head, V = 32+head
                    const int qsoff = lbase + (int)(QKV_W * 4) + head * 16 * 1024;
                    // Q and K are projected with swapped MFMA operands: their accumulators come out as (channels 4*lg + e,
                    // row l15) — the fragments S^T = K Q^T wants — and V in the plain layout P V wants, so this wave's head
                    // runs projection -> scores -> softmax -> P V entirely in registers: no Q/K/V planes, no barrier here.
                    gemm_phase<3, 16, 2, false>(acc, X + l15 * LDX + lg * 4, LDX, rsrc, voff, qsoff, 16 * 16 * 1024, g_qkv,
                                                         qsoff, 16 * 16 * 1024);
                    // out-projection fragments of this chunk fly during the attention
                    ring_prefetch<2>(g_o, rsrc, voff, lbase + (int)(WO_W * 4) + ((wave * 2) * 16 + c * 8) * 1024, 16 * 1024);
                    const f32x4 bq = *reinterpret_cast<const f32x4*>(LW + QKV_B + head * 16 + lg * 4);
                    const f32x4 bk = *reinterpret_cast<const f32x4*>(LW + QKV_B + D + head * 16 + lg * 4);
                    const float bv = LW[QKV_B + 2 * D + head * 16 + l15];
                    f32x4 qt[RB], kt[RB], vv[RB];
#pragma unroll
                    for (int r = 0; r < RB; ++r) {
                        qt[r] = acc[r][0] + bq;
                        kt[r] = acc[r][1] + bk;
                        vv[r] = acc[r][2] + bv;
                    }
                    attention_head_regs<LDC>(qt, kt, vv, Qc, wave * 16, lane);
                }
                __syncthreads();
                // the next consumer's fragments go out before this phase's MFMAs: chunk 1's QKV, or the first FFN chunk
                if (c == 0)
                    ring_prefetch<3>(g_qkv, rsrc, voff, lbase + (int)(QKV_W * 4) + (8 + wave) * 16 * 1024, 16 * 16 * 1024);
                else
                    ring_prefetch<2>(g_f, rsrc, voff, lbase + (int)(W1_W * 4) + (wave * 2) * 16 * 1024, 16 * 1024);
                // out-projection partial: acc_o += O_chunk[48 x 128] * Wo[:, 128c .. 128c+127]^T
                {
                    const int osoff = lbase + (int)(WO_W * 4) + ((wave * 2) * 16 + c * 8) * 1024;
                    gemm_phase<2, 8, 0, false>(acc_o, Qc + l15 * LDC + lg * 4, LDC, rsrc, voff, osoff, 16 * 1024, g_o, osoff, 16 * 1024);
                }
                __syncthreads();
            }
            // residual + bias, then LayerNorm1
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int col = (wave * 2 + n) * 16 + l15;
                const float bv = LW[WO_B + col];
#pragma unroll
                for (int r = 0; r < RB; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) X[(r * 16 + lg * 4 + e) * LDX + col] += acc_o[r][n][e] + bv;
            }
            __syncthreads();
            layernorm_rows16<fz::RP, fz::LDX>(X, LW + G1, LW + BE1, wave, lane);
            __syncthreads();
            // ---- feed-forward block: hidden processed in 4 chunks of 256, second GEMM accumulates in registers -----
            float* Hc = C;
            f32x4 acc_f[RB][2];
            zero_acc<2>(acc_f);
#pragma unroll 1
            for (int f = 0; f < 4; ++f) {
                {
                    f32x4 acc[RB][2];
                    zero_acc<2>(acc);
                    const int nb0 = f * 16 + wave * 2;
                    const int w1off = lbase + (int)(W1_W * 4) + nb0 * 16 * 1024;
                    const int w2off = lbase + (int)(W2_W * 4) + ((wave * 2) * 64 + f * 16) * 1024;
                    // chained: the tail of linear1(f) primes the ring with linear2(f)'s first fragments
                    gemm_phase<2, 16, 0, false>(acc, X + l15 * LDX + lg * 4, LDX, rsrc, voff, w1off, 16 * 1024, g_f, w2off, 64 * 1024);
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const int col = (wave * 2 + n) * 16 + l15;
                        const float bv = LW[W1_B + f * 256 + col];
#pragma unroll
                        for (int r = 0; r < RB; ++r)
#pragma unroll
                            for (int e = 0; e < 4; ++e) Hc[(r * 16 + lg * 4 + e) * LDX + col] = fmaxf(acc[r][n][e] + bv, 0.f);
                    }
                }
                __syncthreads();
                {
                    const int w2off = lbase + (int)(W2_W * 4) + ((wave * 2) * 64 + f * 16) * 1024;
                    // ... and the tail of linear2(f) primes it with linear1(f+1)'s (its own again after the last chunk)
                    const int nxt = f < 3 ? lbase + (int)(W1_W * 4) + ((f + 1) * 16 + wave * 2) * 16 * 1024 : w2off;
                    gemm_phase<2, 16, 0, false>(acc_f, Hc + l15 * LDX + lg * 4, LDX, rsrc, voff, w2off, 64 * 1024, g_f, nxt,
                                      f < 3 ? 16 * 1024 : 64 * 1024);
                }
                __syncthreads();
            }
            // next layer's first QKV fragments (or the RNN input projection's) fly during the epilogue + LayerNorm2
            if (layer + 1 < L)
                ring_prefetch<3>(g_qkv, rsrc, voff, lbase + (int)(LAYER_FLOATS * 4) + (int)(QKV_W * 4) + wave * 16 * 1024,
                                 16 * 16 * 1024);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int col = (wave * 2 + n) * 16 + l15;
                const float bv = LW[W2_B + col];
#pragma unroll
                for (int r = 0; r < RB; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) X[(r * 16 + lg * 4 + e) * LDX + col] += acc_f[r][n][e] + bv;
            }
            __syncthreads();
            layernorm_rows16<fz::RP, fz::LDX>(X, LW + G2, LW + BE2, wave, lane);
            __syncthreads();
        }
        // ---- RNN input projection (:99, first half of nn.RNN): IH = X W_ih^T + (b_ih + b_hh), rows 0..T-1 -> HBM ----
        if (ih_out) {
            f32x4 acc[RB][4];
            zero_acc<4>(acc);
            const int isoff = ih_off_b + (wave * 4) * 16 * 1024;
            WRing<4> g_ih;   // once per window: primed in place (one exposed L2 round trip per window)
            ring_prefetch<4>(g_ih, rsrc, voff, isoff, 16 * 1024);

            gemm_phase<4, 16, 0, false>(acc, X + l15 * LDX + lg * 4, LDX, rsrc, voff, isoff, 16 * 1024, g_ih, isoff, 16 * 1024);
            float* io = ih_out + (size_t)win * T * R;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = (wave * 4 + n) * 16 + l15;
                const float bv = wts[ih_off_b / 4 + R * D + col];
#pragma unroll
                for (int r = 0; r < RB; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int row = r * 16 + lg * 4 + e;
                        if (row < T) io[(size_t)row * R + col] = acc[r][n][e] + bv;
                    }
            }
        }
        // ---- arm the RNN hand-off: this window's rows of HALL start as the all-ones sentinel (saves a 21-MB memset) ---
        if (hall_sentinel) {
            uint4* hp = reinterpret_cast<uint4*>(hall_sentinel + (size_t)win * T * R);
            for (int i = tid; i < T * (R / 4); i += THREADS) hp[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
        }
        // ---- encoder output rows 0..T-1 -> HBM (only when a caller wants it) ---------------------------------------
        if (xout) {
            float* out = xout + (size_t)win * T * D;
            for (int i = tid; i < T * (D / 4); i += THREADS) {
                const int r = i / (D / 4), c4 = i - r * (D / 4);
                *reinterpret_cast<float4*>(out + (size_t)r * D + c4 * 4) = *reinterpret_cast<const float4*>(X + r * LDX + c4 * 4);
            }
        }
        __syncthreads();
    }
}

hipError_t launch_fused_encoder(const Dims& d, const float* fused_w, const float* x_imu, const float* x_s,
                                const float* keep_mask, float keep_scale, float* xout, float* ih_out, float* hall_sentinel,
                                int B, int T, int num_cus, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (hipError_t e = dynamic_lds<fused_encoder_kernel>(fz::LDS_BYTES)) return e;
    const int grid = B < num_cus ? B : num_cus;
    float* iho = fused_has_rnn_ih(d) ? ih_out : nullptr;
    hipLaunchKernelGGL(fused_encoder_kernel, dim3(grid), dim3(fz::THREADS), fz::LDS_BYTES, s, fused_w, x_imu, x_s, keep_mask, keep_scale,
                       xout, iho, reinterpret_cast<unsigned*>(hall_sentinel), B, T, d.n_imu_total, d.S, d.L,
                       (int)(fused_packed_floats(d) * 4), (int)(fused_ih_off(d) * 4), FusedTrain{});
    return hipGetLastError();
}

// "fusedh": the one-window kernel with the hybrid row tiling (the design and the body: tip_fused_h.h)
__device__ unsigned long long g_fh_trace[64];      // measurement only (TIP_FUSEDH_TRACE=1)
__device__ unsigned long long g_fh_wg[2 * 1024];

template <bool TRACE, bool TR, bool LIVE = false>
__global__ __launch_bounds__(fz::THREADS) void fused_encoder_h_kernel(
    const float* __restrict__ wts, const float* __restrict__ x_imu, const float* __restrict__ x_s,
    const float* __restrict__ keep_mask, float keep_scale, float* __restrict__ xout, float* __restrict__ ih_out,
    unsigned* __restrict__ hall_sentinel, int B, int T, int NI, int S, int L, int wbytes, int ih_off_b, FusedEncArgs<LIVE> tr) {
    using Ctl = FhGridStride;
    const Ctl ctl{};
#include "tip_fused_h_body.inc"
}
#undef FH_STAMP

hipError_t launch_fused_encoder_h(const Dims& d, const float* fused_w, const float* x_imu, const float* x_s,
                                  const float* keep_mask, float keep_scale, float* xout, float* ih_out, float* hall_sentinel,
                                  int B, int T, int num_cus, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (hipError_t e = dynamic_lds<fused_encoder_h_kernel<false, false>, fused_encoder_h_kernel<true, false>>(fz::LDS_BYTES)) return e;
    const int grid = B < num_cus ? B : num_cus;
    float* iho = fused_has_rnn_ih(d) ? ih_out : nullptr;
    if (measure_switches().fusedh_trace)
        hipLaunchKernelGGL((fused_encoder_h_kernel<true, false>), dim3(grid), dim3(fz::THREADS), fz::LDS_BYTES, s, fused_w, x_imu, x_s, keep_mask,
                           keep_scale, xout, iho, reinterpret_cast<unsigned*>(hall_sentinel), B, T, d.n_imu_total, d.S, d.L,
                           (int)(fused_packed_floats(d) * 4), (int)(fused_ih_off(d) * 4), FusedTrain{});
    else
        hipLaunchKernelGGL((fused_encoder_h_kernel<false, false>), dim3(grid), dim3(fz::THREADS), fz::LDS_BYTES, s, fused_w, x_imu, x_s, keep_mask,
                           keep_scale, xout, iho, reinterpret_cast<unsigned*>(hall_sentinel), B, T, d.n_imu_total, d.S, d.L,
                           (int)(fused_packed_floats(d) * 4), (int)(fused_ih_off(d) * 4), FusedTrain{});
    return hipGetLastError();
}

// training forward on the hybrid tiling
hipError_t launch_fused_train_h(const Dims& d, const float* fused_w, const float* x_imu, const float* x_s, const float* keep_mask,
                                float keep_scale, float* ih_out, float* hall_sentinel, const FusedTrain& tr, int B, int T,
                                int num_cus, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (!fused_supported(d, T) || !fused_has_rnn_ih(d)) return hipErrorInvalidValue;
    if (hipError_t e = dynamic_lds<fused_encoder_h_kernel<false, true>, fused_encoder_h_kernel<true, true>>(fz::LDS_BYTES)) return e;
    const int grid = B < num_cus ? B : num_cus;
    if (measure_switches().fusedh_trace) {   // measurement: the same phase stamps as the inference kernel (tools/fh_trace.py --train)
        hipLaunchKernelGGL((fused_encoder_h_kernel<true, true>), dim3(grid), dim3(fz::THREADS), fz::LDS_BYTES, s, fused_w, x_imu, x_s,
                           keep_mask, keep_scale, (float*)nullptr, ih_out, reinterpret_cast<unsigned*>(hall_sentinel), B, T, d.n_imu_total,
                           d.S, d.L, (int)(fused_packed_floats(d) * 4), (int)(fused_ih_off(d) * 4), tr);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((fused_encoder_h_kernel<false, true>), dim3(grid), dim3(fz::THREADS), fz::LDS_BYTES, s, fused_w, x_imu, x_s,
                       keep_mask, keep_scale, (float*)nullptr, ih_out, reinterpret_cast<unsigned*>(hall_sentinel), B, T, d.n_imu_total,
                       d.S, d.L, (int)(fused_packed_floats(d) * 4), (int)(fused_ih_off(d) * 4), tr);
    return hipGetLastError();
}

// the deployed forward (tip_forward_live): dropout sites and keep mask live, nothing stashed, inference outputs
hipError_t launch_fused_live_h(const Dims& d, const float* fused_w, const float* x_imu, const float* x_s, const float* keep_mask,
                               float keep_scale, float* xout, float* ih_out, float* hall_sentinel, const FusedTrain& tr,
                               const LiveArgs& lv, int B, int T, int num_cus, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (!fused_supported(d, T) || !fused_has_rnn_ih(d)) return hipErrorInvalidValue;
    if (hipError_t e = dynamic_lds<fused_encoder_h_kernel<false, false, true>>(fz::LDS_BYTES)) return e;
    const int grid = B < num_cus ? B : num_cus;
    LiveTrain lt;
    static_cast<FusedTrain&>(lt) = tr;
    lt.lv = lv;
    hipLaunchKernelGGL((fused_encoder_h_kernel<false, false, true>), dim3(grid), dim3(fz::THREADS), fz::LDS_BYTES, s, fused_w, x_imu, x_s,
                       keep_mask, keep_scale, xout, ih_out, reinterpret_cast<unsigned*>(hall_sentinel), B, T, d.n_imu_total, d.S, d.L,
                       (int)(fused_packed_floats(d) * 4), (int)(fused_ih_off(d) * 4), lt);
    return hipGetLastError();
}

}  // namespace tip
extern "C" int tip_debug_read_fh_wg(unsigned long long* out, int n) {
    if (!out || n < 0 || n > 2048 + 5 * 1024) return -1;
    if (n > 2048 && tip::read_round_wg(out + 2048, n - 2048) != hipSuccess) return -5;   // the one-launch round's table behind this one
    if (n > 2048) n = 2048;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(tip::g_fh_wg), sizeof(unsigned long long) * n) == hipSuccess ? 0 : -5;
}
extern "C" int tip_debug_read_fh_trace(unsigned long long* out, int n) {
    if (!out || n < 0 || n > 64) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(tip::g_fh_trace), sizeof(unsigned long long) * n) == hipSuccess ? 0 : -5;
}
namespace tip {
// =====================================================================================================================
// Training step, backward of one encoder layer's feed-forward block, fused per window.
//   dy = dL/d(layer output)  ->  LayerNorm2 backward  ->  dz2 (kept: it is also the residual path into the block's input)
//   dff2 = dz2 * keep3                      (gradient into linear2's output; also linear2's bias-gradient rows)
//   dpre = (dff2 W2) * [hid > 0] / (1 - p)  (hid was saved AFTER ReLU and dropout: its sign is the gate)
//   dx1  = dz2 + dpre W1
// Same structure as the forward FFN phases of fused_encoder_kernel — activations [48 x 256] resident in LDS, the hidden
// dimension walked in 4 chunks of 256, weight fragments of W2^T ([F][D]) and W1^T ([D][F]) streamed from the backward
// image with the same ring/offset scheme as W1 / W2 in the forward — so the two 10 240-row GEMMs and the LayerNorm
// kernel of the layer-by-layer backward (and the HBM round trips between them) become one launch.
// dff2 and dpre still go to HBM: the weight-gradient GEMMs (reduction over all rows of the batch) read them.
// =====================================================================================================================
namespace fb {
constexpr size_t W2T = 0;                                  // [F][D] fragments: B operand of dhid = dff2 W2
constexpr size_t W1T = W2T + (size_t)fz::F * fz::D;        // [D][F] fragments: B operand of dx1 = dpre W1
constexpr size_t WOT = W1T + (size_t)fz::D * fz::F;        // [D][D]  fragments of Wo^T:   datt = datt_o Wo
constexpr size_t WQT = WOT + (size_t)fz::D * fz::D;        // [D][3D] fragments of Wqkv^T: dx_in = dqkv Wqkv
constexpr size_t LAYER_FLOATS2 = WQT + (size_t)fz::D * 3 * fz::D;   // per-layer stride of the backward image

}  // namespace fb

size_t fused_bwd_image_floats(const Dims& d) {
    if (fused_packed_floats(d) == 0) return 0;
    return (size_t)d.L * fb::LAYER_FLOATS2 + fz::TAIL_PAD;
}

void fused_bwd_pack_ops(const Dims& d, const float* const* t, size_t base, std::vector<PackOp>& ops) {
    using namespace fz;
    for (int l = 0; l < d.L; ++l) {
        const float* const* lw = t + 2 + 12 * l;
        const size_t L = base + (size_t)l * fb::LAYER_FLOATS2;
        ops.push_back(frag_op(lw[6], L + fb::W2T, F, D, F, D, 1));          // linear2.weight is [D][F]: logical W2^T [F][D]
        ops.push_back(frag_op(lw[4], L + fb::W1T, D, F, D, F, 1));          // linear1.weight is [F][D]: logical W1^T [D][F]
        ops.push_back(frag_op(lw[2], L + fb::WOT, D, D, D, D, 1));          // out_proj.weight [D][D]: logical Wo^T
        ops.push_back(frag_op(lw[0], L + fb::WQT, D, 3 * D, D, 3 * D, 1));  // in_proj_weight [3D][D]: logical Wqkv^T [D][3D]
    }
}

// measurement only (TIP_BWD_TRACE=1): s_memtime stamps of workgroup 0 / thread 0 at the phase boundaries of the two fused
// backward kernels ([0..7] ffn_bwd, [8..15] attn_bwd), read back with tip_debug_read_bwd_trace() (tools/bwd_trace.py)
__device__ unsigned long long g_bwd_trace[16];
__device__ __forceinline__ void bwd_stamp(int on, int slot) {
    if (on && blockIdx.x == 0 && threadIdx.x == 0) g_bwd_trace[slot] = __builtin_amdgcn_s_memtime();
}


// BITS: the ReLU / dropout gates come as the bit array the fused training forward wrote (hidden_to_hbm), staged into LDS once per
// window; otherwise (layer-by-layer forward) from the saved fp32 hidden rows.
constexpr int kGateLd = 36;   // dwords per row of the LDS copy (32 + 4: the 16 rows a lane group reads sit on distinct bank quads)
template <bool BITS>
__global__ __launch_bounds__(fz::THREADS) void ffn_bwd_kernel(FfnBwdArgs a, int B, int T) {
    using namespace fz;
    using namespace fzh;   // hybrid row tiling as in fused_encoder_h_kernel: rows 0-31 on 16x16x4, rows 32-39 on 4x4x1 MFMAs, nothing on pad rows
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* G = smem;                       // dy -> dz2 -> dx1
    float* Mb = smem + RP * LDX;           // dff2 (masked dz2)
    float* Hc = smem + 2 * RP * LDX;       // dpre chunk; scratch for the LayerNorm parameter partials before that
    unsigned* GB = reinterpret_cast<unsigned*>(smem + 3 * RP * LDX);   // BITS: this window's gate bits [RP][kGateLd], dword f*8 + half*4 + e
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wimg), 0, a.wbytes, 0x00020000);
    const int voff = lane * 16;
    const int lbase = (int)(((size_t)a.layer * fb::LAYER_FLOATS2) * 4);
    auto am = [&](int ld) { return l15 * ld + lg * 4; };                       // this lane's LDS offsets: 16-row blocks / tail blocks
    auto at = [&](int ld) { return (TAIL0 + (lane & 3)) * ld + lg * 4; };
    // the saved hidden activations through a buffer descriptor (byte offsets must fit 32 bits: checked by the launcher)
    const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.hid), 0, a.hid_bytes, 0x00020000);

    const unsigned dkey = tip_drop_key_s(a.seed, a.site);
    for (int win = blockIdx.x; win < B; win += gridDim.x) {
        const size_t grow0 = (size_t)win * T;
        bwd_stamp(a.trace, 0);
        WRing<2> g_f;
        ring_prefetch<2>(g_f, rsrc, voff, lbase + (int)(fb::W2T * 4) + (wave * 2) * 16 * 1024, 16 * 1024);
        u32x4 gq = {0u, 0u, 0u, 0u};   // BITS: 16 bytes of this window's 40 x 128 B of gate bits per thread (tid < 8 T), to LDS below
        if (BITS && tid < 8 * T) gq = *reinterpret_cast<const u32x4*>(a.gbits + (grow0 + (tid >> 3)) * 32 + (tid & 7) * 4);
        // ---- LayerNorm2 backward, one wave per row (rows w, w+8, ...) ------------------------------------------------------
        {
            const float4 gg = *reinterpret_cast<const float4*>(a.g2 + lane * 4);
            float4 dg = make_float4(0.f, 0.f, 0.f, 0.f), db = dg, dm = dg;
            // every row's operands are requested BEFORE the first row is worked on: written as one load -> compute -> store body
            // per row, the stores of row i stood between the optimiser and the loads of row i + 1 (it may not move a load across a
            // store it cannot prove disjoint), and the phase was three HBM round trips long (14 000 cycles for 5 rows per wave)
            constexpr int NR = RP / 8;
            float4 zq[NR], dq_[NR];
            float2 sq_[NR];
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int r = wave + 8 * i;
                const size_t gr = grow0 + (r < T ? r : 0);      // pad rows: a valid address, the values are not used
                zq[i] = *reinterpret_cast<const float4*>(a.z2 + gr * D + lane * 4);
                dq_[i] = *reinterpret_cast<const float4*>(a.dy + gr * D + lane * 4);
                sq_[i] = *reinterpret_cast<const float2*>(a.st2 + gr * 2);
            }
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int r = wave + 8 * i;
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f), m = o;
                if (r < T) {
                    const size_t gr = grow0 + r;
                    const float4 zv = zq[i];
                    const float4 dyv = dq_[i];
                    const float mean = sq_[i].x, rstd = sq_[i].y;
                    float4 xh;
                    xh.x = (zv.x - mean) * rstd; xh.y = (zv.y - mean) * rstd; xh.z = (zv.z - mean) * rstd; xh.w = (zv.w - mean) * rstd;
                    const float ax = dyv.x * gg.x, ay = dyv.y * gg.y, az = dyv.z * gg.z, aw = dyv.w * gg.w;
                    const float m1 = wsum((ax + ay) + (az + aw)) * (1.f / D);
                    const float m2 = wsum((ax * xh.x + ay * xh.y) + (az * xh.z + aw * xh.w)) * (1.f / D);
                    dg.x += dyv.x * xh.x; dg.y += dyv.y * xh.y; dg.z += dyv.z * xh.z; dg.w += dyv.w * xh.w;
                    db.x += dyv.x; db.y += dyv.y; db.z += dyv.z; db.w += dyv.w;
                    o.x = rstd * (ax - m1 - xh.x * m2); o.y = rstd * (ay - m1 - xh.y * m2);
                    o.z = rstd * (az - m1 - xh.z * m2); o.w = rstd * (aw - m1 - xh.w * m2);
                    m = o;
                    if (a.thresh) {
                        const unsigned long long idx = gr * D + lane * 4;
                        m.x = tip_drop_hash_k(dkey, idx) >= a.thresh ? o.x * a.scale : 0.f;
                        m.y = tip_drop_hash_k(dkey, idx + 1) >= a.thresh ? o.y * a.scale : 0.f;
                        m.z = tip_drop_hash_k(dkey, idx + 2) >= a.thresh ? o.z * a.scale : 0.f;
                        m.w = tip_drop_hash_k(dkey, idx + 3) >= a.thresh ? o.w * a.scale : 0.f;
                    }
                    *reinterpret_cast<float4*>(a.dff2 + gr * D + lane * 4) = m;
                    dm.x += m.x; dm.y += m.y; dm.z += m.z; dm.w += m.w;
                }
                *reinterpret_cast<float4*>(G + r * LDX + lane * 4) = o;      // padded rows: zeros
                *reinterpret_cast<float4*>(Mb + r * LDX + lane * 4) = m;
            }
            // per-window partials of dgamma2 | dbeta2 | d(linear2 bias): waves -> LDS -> one [3*D] row per window
            float* red = Hc;   // [8 waves][3][D]
            *reinterpret_cast<float4*>(red + (wave * 3 + 0) * D + lane * 4) = dg;
            *reinterpret_cast<float4*>(red + (wave * 3 + 1) * D + lane * 4) = db;
            *reinterpret_cast<float4*>(red + (wave * 3 + 2) * D + lane * 4) = dm;
        }
        if (BITS && tid < 8 * T) {
            // global dwords (f*8 + 2 e + half) -> LDS dwords (f*8 + 4 half + e): a lane's four e of one half are then one 16-byte read
            const int row = tid >> 3, q = tid & 7, fq = q >> 1, e0 = (q & 1) * 2;
            unsigned* g = GB + row * kGateLd + fq * 8;
            g[e0] = gq[0]; g[4 + e0] = gq[1]; g[e0 + 1] = gq[2]; g[4 + e0 + 1] = gq[3];
        }
        __syncthreads();
        for (int i = tid; i < 3 * D; i += THREADS) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) s += Hc[w * 3 * D + i];
            a.lnpart[(size_t)win * (3 * D + F) + i] = s;
        }
        __syncthreads();
        bwd_stamp(a.trace, 1);
        // ---- hidden chunks ------------------------------------------------------------------------------------------------
        f32x4 acc_x[RBM][2], acc_xt[RBT][2];
        zero_acc_h<2>(acc_x, acc_xt);
#pragma unroll 1
        for (int f = 0; f < 4; ++f) {
            {
                f32x4 acc[RBM][2], acct[RBT][2];
                zero_acc_h<2>(acc, acct);
                const int w2off = lbase + (int)(fb::W2T * 4) + (f * 16 + wave * 2) * 16 * 1024;
                const int w1off = lbase + (int)(fb::W1T * 4) + ((wave * 2) * 64 + f * 16) * 1024;
                // The product is computed TRANSPOSED (weights as the A operand): a lane then holds 4 consecutive hidden
                // channels of ONE row, so the ReLU/dropout gate is one 16-byte load of the saved hidden row and the chunk goes
                // to LDS as one 16-byte store per tile.  The gate loads are issued before the MFMAs (buffer loads: opaque to the
                // optimiser, so they stay here) and consumed after.
                f32x4 gate[RBM][2];
                float gatet[RBT][2];   // the tail comes out in the plain orientation: lane (lg, l15) = row 32 + 4 rb + lg, channel l15
                u32x4 gw[RBM];         // BITS: row r*16 + l15, dword e: bit ((wave & 3)*2 + n)*4 + lg is the gate of element (r, n, e)
                unsigned gwt[RBT];     // BITS: row 32 + 4 rb + lg, dword of e = l15 & 3: bit ((wave & 3)*2 + n)*4 + (l15 >> 2)
                if (BITS) {
                    const int half = wave >> 2;
#pragma unroll
                    for (int r = 0; r < RBM; ++r) gw[r] = *reinterpret_cast<const u32x4*>(GB + (r * 16 + l15) * kGateLd + f * 8 + half * 4);
#pragma unroll
                    for (int rb = 0; rb < RBT; ++rb) gwt[rb] = GB[(TAIL0 + 4 * rb + lg) * kGateLd + f * 8 + half * 4 + (l15 & 3)];
                }
                if (!BITS) {
#pragma unroll
                for (int n = 0; n < 2; ++n) {
#pragma unroll
                    for (int r = 0; r < RBM; ++r) {
                        const int row = r * 16 + l15;
                        const long long off = ((long long)(grow0 + (row < T ? row : 0)) * F + f * 256 + (wave * 2 + n) * 16 + lg * 4) * 4;
                        gate[r][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(hrs, (int)off, 0, 0));
                    }
#pragma unroll
                    for (int rb = 0; rb < RBT; ++rb) {
                        const int row = TAIL0 + 4 * rb + lg;
                        const long long off = ((long long)(grow0 + (row < T ? row : 0)) * F + f * 256 + (wave * 2 + n) * 16 + l15) * 4;
                        gatet[rb][n] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(hrs, (int)off, 0, 0));
                    }
                }
                }
                // the tail of this phase primes the ring with the dx1 phase's first fragments
                gemm_phase_h<2, 16, 2, true>(acc, acct, Mb + am(LDX), Mb + at(LDX), LDX, rsrc, voff, w2off, 16 * 1024, g_f, w1off, 64 * 1024);
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    f32x4 bs = {0.f, 0.f, 0.f, 0.f};   // this window's share of linear1's bias gradient: column sums of the chunk
#pragma unroll
                    for (int r = 0; r < RBM; ++r) {
                        const int row = r * 16 + l15;
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool open = BITS ? ((gw[r][e] >> (((wave & 3) * 2 + n) * 4 + lg)) & 1u) != 0u : gate[r][n][e] > 0.f;
                            v[e] = (row < T && open) ? acc[r][n][e] * a.gate_scale : 0.f;
                        }
                        *reinterpret_cast<f32x4*>(Hc + row * LDX + (wave * 2 + n) * 16 + lg * 4) = v;
                        bs += v;
                    }
                    float ts = 0.f;   // rows 32..39: lane (lg, l15) = (row 32 + 4 rb + lg, channel l15) after the tail's reduce-scatter
#pragma unroll
                    for (int rb = 0; rb < RBT; ++rb) {
                        const int row = TAIL0 + 4 * rb + lg;
                        const float x = tail_reduce(acct[rb][n], lg);
                        const bool open = BITS ? ((gwt[rb] >> (((wave & 3) * 2 + n) * 4 + (l15 >> 2))) & 1u) != 0u : gatet[rb][n] > 0.f;
                        const float v = (row < T && open) ? x * a.gate_scale : 0.f;
                        Hc[row * LDX + (wave * 2 + n) * 16 + l15] = v;
                        ts += v;
                    }
                    ts = lg4_sum(ts);   // every lane (any lg, l15): the tail rows' sum of channel l15
                    // the lane holds 4 consecutive hidden channels of rows l15 and 16 + l15: the sum over rows is a butterfly over the 16
                    // lanes that share lg, straight from the registers; the tail's share of channel 4 lg + e sits in lane l15 = 4 lg + e
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x = bs[e];
                        x = row16_sum(x);
                        bs[e] = x + __shfl(ts, (lane & 48) | (lg * 4 + e), 64);
                    }
                    if (l15 == 0)
                        *reinterpret_cast<f32x4*>(a.lnpart + (size_t)win * (3 * D + F) + 3 * D + f * 256 + (wave * 2 + n) * 16 + lg * 4) = bs;
                }
            }
            if (f == 0) bwd_stamp(a.trace, 2);     // first chunk: d(hidden) product done
            __syncthreads();
            if (f == 0) bwd_stamp(a.trace, 3);
            rows_to_hbm_fixed<256>(Hc, LDX, a.dpre + grow0 * F + f * 256, F, T, tid);   // (a counted number of stores in front of the dx1 phase's ring)
            {
                const int w1off = lbase + (int)(fb::W1T * 4) + ((wave * 2) * 64 + f * 16) * 1024;
                const int nxt = f < 3 ? lbase + (int)(fb::W2T * 4) + ((f + 1) * 16 + wave * 2) * 16 * 1024 : w1off;
                if (f == 0) bwd_stamp(a.trace, 4);     // first chunk: rows + bias partials out
                gemm_phase_h<2, 16, 0, true>(acc_x, acc_xt, Hc + am(LDX), Hc + at(LDX), LDX, rsrc, voff, w1off, 64 * 1024, g_f, nxt,
                                             f < 3 ? 16 * 1024 : 64 * 1024);
                if (f == 0) bwd_stamp(a.trace, 5);     // first chunk: dx1 partial product done
            }
            __syncthreads();
        }
        bwd_stamp(a.trace, 6);
        // ---- dx1 = dz2 + dpre W1 -------------------------------------------------------------------------------------------
#pragma unroll
        for (int n = 0; n < 2; ++n) {   // dz2 values read before the first write-back (tip_pgemm.h: `G[i] += v` serialises read -> wait -> write)
            const int col = (wave * 2 + n) * 16 + l15;
            float gr_[RBM][4], gt_[RBT];
#pragma unroll
            for (int r = 0; r < RBM; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) gr_[r][e] = G[(r * 16 + lg * 4 + e) * LDX + col];
#pragma unroll
            for (int rb = 0; rb < RBT; ++rb) gt_[rb] = G[(TAIL0 + 4 * rb + lg) * LDX + col];
#pragma unroll
            for (int r = 0; r < RBM; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) G[(r * 16 + lg * 4 + e) * LDX + col] = gr_[r][e] + acc_x[r][n][e];
#pragma unroll
            for (int rb = 0; rb < RBT; ++rb) G[(TAIL0 + 4 * rb + lg) * LDX + col] = gt_[rb] + tail_reduce(acc_xt[rb][n], lg);
        }
        __syncthreads();
        rows_to_hbm_fixed<D>(G, LDX, a.dx1 + grow0 * D, D, T, tid);
        bwd_stamp(a.trace, 7);
        __syncthreads();
    }
}

hipError_t launch_ffn_bwd(const Dims& d, const FfnBwdArgs& a, int B, int T, int num_cus, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (!fused_supported(d, T) || (long long)B * T * d.F * 4 > 0x7fffffffLL) return hipErrorInvalidValue;
    constexpr int lds = (3 * fz::RP * fz::LDX + fz::RP * kGateLd) * 4;
    static_assert(lds <= 160 * 1024, "LDS of one CU");
    if (hipError_t e = dynamic_lds<ffn_bwd_kernel<false>, ffn_bwd_kernel<true>>(lds)) return e;
    FfnBwdArgs aa = a;
    aa.hid_bytes = (int)((long long)B * T * d.F * 4);
    aa.trace = measure_switches().bwd_trace ? 1 : 0;
    if (aa.gbits) hipLaunchKernelGGL(ffn_bwd_kernel<true>, dim3(B < num_cus ? B : num_cus), dim3(fz::THREADS), lds, s, aa, B, T);
    else hipLaunchKernelGGL(ffn_bwd_kernel<false>, dim3(B < num_cus ? B : num_cus), dim3(fz::THREADS), lds, s, aa, B, T);
    return hipGetLastError();
}

// =====================================================================================================================
// Training step, backward of one encoder layer's ATTENTION block, fused per window:
//   dx1 = dL/d(LayerNorm1 output)  ->  LayerNorm1 backward  ->  dz1 (to HBM: it is also the residual path)
//   datt_o = dz1 * keep1 (gradient into out_proj's output)  ->  dO = datt_o Wo, per head, in registers, in BOTH layouts
//   attention backward per head in registers (as tip_attn.hip, mattn_bwd_kernel) -> dq | dk | dv planes in LDS (+ HBM)
//   dx_in = dz1 + [dq | dk | dv] W_qkv
// One wave owns one head end to end; 2 chunks of 8 heads as in the forward.  datt_o and dqkv also go to HBM for the
// weight-gradient GEMMs.
// =====================================================================================================================

// DROP: attention / out-proj dropout on (a.thresh != 0).  A template parameter, and the masked elements below are SELECTS, not branches:
// with `if (valid) { ... }` around each element (and a uniform `if (a.thresh)` inside it) the attention part was 450 basic blocks,
// MFMA -> branch -> exp -> MFMA strictly in program order, nothing for the scheduler to overlap (the heads ran at 50 % of their MFMA time).
template <bool DROP>
__global__ __launch_bounds__(fz::THREADS) void attn_bwd_kernel(AttnBwdArgs a, int B, int T) {
    using namespace fz;
    constexpr int LDT = 20;                             // per-wave transposition tiles [48][16 + 4]
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Mb = smem;                                   // datt_o [48][260]
    float* Sc = smem + RP * LDX;                        // per-wave scratch: Q tile | K tile (LayerNorm partials before that)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wimg), 0, a.wbytes, 0x00020000);
    const int voff = lane * 16;
    const int lbase = (int)(((size_t)a.layer * fb::LAYER_FLOATS2) * 4);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    float* Qs = Sc + wave * (3 * RP * LDT);             // this wave's head: Q rows [48][16] (row-major) ...
    float* Ks = Qs + RP * LDT;                          // ... and K rows: read back as (row 4*lg + e, channel l15) B fragments
    float* Gs = Ks + RP * LDT;                          // dO tile: written in the accumulator layout, read back as row fragments
    float* Ts = Gs;                                     // ... and, once it has been read, the P | dS transposition tiles [2][16][20]
    const unsigned dkey0 = tip_drop_key_s(a.seed, a.site0), dkey1 = tip_drop_key_s(a.seed, a.site1);

    for (int win = blockIdx.x; win < B; win += gridDim.x) {
        const size_t grow0 = (size_t)win * T;
        bwd_stamp(a.trace, 8);
        WRing<1> g_o;   // Wo^T fragments of head c*8 + wave
        ring_prefetch<1>(g_o, rsrc, voff, lbase + (int)(fb::WOT * 4) + wave * 16 * 1024, 0);
        // ---- LayerNorm1 backward --------------------------------------------------------------------------------------------
        {
            const float4 gg = *reinterpret_cast<const float4*>(a.g1 + lane * 4);
            float4 dg = make_float4(0.f, 0.f, 0.f, 0.f), db = dg, dm = dg;
            // all rows' operands first (ffn_bwd_kernel: the stores of row i otherwise fence the loads of row i + 1)
            constexpr int NR = RP / 8;
            float4 zq[NR], dq_[NR];
            float2 sq_[NR];
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int r = wave + 8 * i;
                const size_t gr = grow0 + (r < T ? r : 0);
                zq[i] = *reinterpret_cast<const float4*>(a.z1 + gr * D + lane * 4);
                dq_[i] = *reinterpret_cast<const float4*>(a.dx1 + gr * D + lane * 4);
                sq_[i] = *reinterpret_cast<const float2*>(a.st1 + gr * 2);
            }
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int r = wave + 8 * i;
                float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < T) {
                    const size_t gr = grow0 + r;
                    const float4 zv = zq[i];
                    const float4 dyv = dq_[i];
                    const float mean = sq_[i].x, rstd = sq_[i].y;
                    float4 xh;
                    xh.x = (zv.x - mean) * rstd; xh.y = (zv.y - mean) * rstd; xh.z = (zv.z - mean) * rstd; xh.w = (zv.w - mean) * rstd;
                    const float ax = dyv.x * gg.x, ay = dyv.y * gg.y, az = dyv.z * gg.z, aw = dyv.w * gg.w;
                    const float m1 = wsum((ax + ay) + (az + aw)) * (1.f / D);
                    const float m2 = wsum((ax * xh.x + ay * xh.y) + (az * xh.z + aw * xh.w)) * (1.f / D);
                    dg.x += dyv.x * xh.x; dg.y += dyv.y * xh.y; dg.z += dyv.z * xh.z; dg.w += dyv.w * xh.w;
                    db.x += dyv.x; db.y += dyv.y; db.z += dyv.z; db.w += dyv.w;
                    float4 o;
                    o.x = rstd * (ax - m1 - xh.x * m2); o.y = rstd * (ay - m1 - xh.y * m2);
                    o.z = rstd * (az - m1 - xh.z * m2); o.w = rstd * (aw - m1 - xh.w * m2);
                    *reinterpret_cast<float4*>(a.dz1 + gr * D + lane * 4) = o;
                    m = o;
                    if (DROP) {
                        const unsigned long long idx = gr * D + lane * 4;
                        m.x = tip_drop_hash_k(dkey1, idx) >= a.thresh ? o.x * a.scale : 0.f;
                        m.y = tip_drop_hash_k(dkey1, idx + 1) >= a.thresh ? o.y * a.scale : 0.f;
                        m.z = tip_drop_hash_k(dkey1, idx + 2) >= a.thresh ? o.z * a.scale : 0.f;
                        m.w = tip_drop_hash_k(dkey1, idx + 3) >= a.thresh ? o.w * a.scale : 0.f;
                    }
                    *reinterpret_cast<float4*>(a.datt_o + gr * D + lane * 4) = m;
                    dm.x += m.x; dm.y += m.y; dm.z += m.z; dm.w += m.w;
                }
                *reinterpret_cast<float4*>(Mb + r * LDX + lane * 4) = m;      // padded rows: zeros
            }
            float* red = Sc;   // [8 waves][3][D] = 6144 floats
            *reinterpret_cast<float4*>(red + (wave * 3 + 0) * D + lane * 4) = dg;
            *reinterpret_cast<float4*>(red + (wave * 3 + 1) * D + lane * 4) = db;
            *reinterpret_cast<float4*>(red + (wave * 3 + 2) * D + lane * 4) = dm;
        }
        __syncthreads();
        for (int i = tid; i < 3 * D; i += THREADS) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) s += Sc[w * 3 * D + i];
            a.lnpart[(size_t)win * 6 * D + i] = s;
        }
        __syncthreads();

        bwd_stamp(a.trace, 9);
        // ---- per head (no workgroup barrier in here: a wave only touches Mb (read), its own scratch and its own HBM columns) ---
#pragma unroll 1
        for (int c = 0; c < 2; ++c) {
            bwd_stamp(a.trace, 10 + c);
            const int head = c * 8 + wave;
            const unsigned long long bh = (unsigned long long)win * H + head;
            const __amdgpu_buffer_rsrc_t q_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.qkv) + grow0 * (3 * D), 0, T * 3 * D * 4, 0x00020000);
            const __amdgpu_buffer_rsrc_t o_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.att) + grow0 * D, 0, T * D * 4, 0x00020000);
            const __amdgpu_buffer_rsrc_t st_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.ast) + bh * T * 2, 0, T * 8, 0x00020000);
            // this window's dq | dk | dv rows as a buffer whose extent is T rows: stores to the padded rows are dropped by the
            // hardware's range check instead of by a branch around every store (each one ended a basic block)
            const __amdgpu_buffer_rsrc_t dq_rs = __builtin_amdgcn_make_buffer_rsrc(a.dqkv + grow0 * (3 * D), 0, T * 3 * D * 4, 0x00020000);
            const int dq_col = (head * 16 + l15) * 4;
            // q, k, v, O row fragments and the softmax statistics are requested before the dO product
            f32x4 qf[RB], kf[RB], vf[RB], of[RB];
            float mq[RB], iq[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int row = r * 16 + l15;
                // rows >= T: out of the buffers' extent -> zeros, no branch
                const int qo = row * (3 * D * 4) + head * 64 + lg * 16;
                qf[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(q_rs, qo, 0, 0));
                kf[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(q_rs, qo + D * 4, 0, 0));
                vf[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(q_rs, qo + 2 * D * 4, 0, 0));
                of[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(o_rs, row * (D * 4) + head * 64 + lg * 16, 0, 0));
                typedef float tf2 __attribute__((ext_vector_type(2)));
                const tf2 mi = __builtin_bit_cast(tf2, __builtin_amdgcn_raw_buffer_load_b64(st_rs, row * 8, 0, 0));
                mq[r] = mi[0];
                iq[r] = mi[1];
            }
            // dO of this head: [48 x 16] = datt_o [48 x 256] * Wo^T(:, head): gp = accumulator layout (rows 4*lg + e, channel l15);
            // gs = the same tile as row fragments (row l15, channels 4*lg + e), obtained through the wave's scratch
            f32x4 gs[RB], gp[RB];
            {
                f32x4 acc[RB][1];
                zero_acc<1>(acc);
                const int osoff = lbase + (int)(fb::WOT * 4) + head * 16 * 1024;
                const int nxt = c == 0 ? lbase + (int)(fb::WOT * 4) + (8 + wave) * 16 * 1024 : osoff;
                gemm_phase<1, 16>(acc, Mb + l15 * LDX + lg * 4, LDX, rsrc, voff, osoff, 0, g_o, nxt, 0);
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    gp[r] = acc[r][0];
#pragma unroll
                    for (int e = 0; e < 4; ++e) Gs[(r * 16 + lg * 4 + e) * LDT + l15] = gp[r][e];
                }
            }
            // Q and K rows through the wave's scratch: written as row fragments, read back transposed (row 4*lg + e, channel l15)
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                *reinterpret_cast<f32x4*>(Qs + (r * 16 + l15) * LDT + lg * 4) = qf[r];
                *reinterpret_cast<f32x4*>(Ks + (r * 16 + l15) * LDT + lg * 4) = kf[r];
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < RB; ++r) gs[r] = *reinterpret_cast<const f32x4*>(Gs + (r * 16 + l15) * LDT + lg * 4);
            float dd[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                float d_ = (gs[r][0] * of[r][0] + gs[r][1] * of[r][1]) + (gs[r][2] * of[r][2] + gs[r][3] * of[r][3]);
                d_ = lg4_sum(d_);
                dd[r] = d_;
            }
            f32x4 dk[RB], dv[RB];
            float sq = 0.f;   // this lane's share of the in-projection bias gradient (column sums of dq)
#pragma unroll
            for (int r = 0; r < RB; ++r) dk[r] = dv[r] = zero4;
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int q = r * 16 + l15;
                f32x4 dq = zero4;
#pragma unroll
                for (int cb = 0; cb <= r; ++cb) {
                    // (key 4*lg + e, query l15): scores and dP once, on the matrix pipe
                    f32x4 s1 = zero4, p1 = zero4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[cb][e], qf[r][e], s1, 0, 0, 0);
                        p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[cb][e], gs[r][e], p1, 0, 0, 0);
                    }
                    f32x4 pd, ds;   // dropped probabilities, dS: the operands of dV / dK in the transposed layout
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int kk = cb * 16 + lg * 4 + e;
                        // masked (kk > q) or padded (q >= T) elements: the select sits on the exponent (exp(-inf) = 0 -> p = 0 -> v = 0
                        // exactly), where both sides are cheap; a select on the RESULT is turned back into a branch around the exp
                        const float p = __expf((kk <= q && q < T) ? s1[e] * a.q_scale - mq[r] : -INFINITY) * iq[r];
                        float kf_ = 1.f;
                        if (DROP) kf_ = tip_drop_hash_k(dkey0, (bh * T + q) * T + kk) >= a.thresh ? a.scale : 0.f;
                        pd[e] = p * kf_;
                        ds[e] = p * (p1[e] * kf_ - dd[r]);
                    }
                    // The same two tiles with the roles of the lane and the register swapped — (query 4*lg + e, key l15), what dV and
                    // dK reduce over — through the wave's scratch (the dO tile's, free since gs was read): 8 LDS writes + 2 reads.
                    // Vector-ALU work does not issue under fp32 MFMAs on this part (tools/probes/coissue_probe.hip), LDS traffic
                    // does: until round 5 this layout was COMPUTED a second time (8 MFMAs, 4 exponentials, 4 dropout hashes and 12
                    // cross-lane reads per block pair), and the heads ran at 52 % of their MFMA time.
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        Ts[(lg * 4 + e) * LDT + l15] = pd[e];
                        Ts[(16 + lg * 4 + e) * LDT + l15] = ds[e];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        dq = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[e], Ks[(cb * 16 + lg * 4 + e) * LDT + l15], dq, 0, 0, 0);
                    __builtin_amdgcn_wave_barrier();
                    const f32x4 pdt = *reinterpret_cast<const f32x4*>(Ts + l15 * LDT + lg * 4);
                    const f32x4 dst = *reinterpret_cast<const f32x4*>(Ts + (16 + l15) * LDT + lg * 4);
                    __builtin_amdgcn_wave_barrier();   // (the next block pair's writes stay behind these reads)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int qq = r * 16 + lg * 4 + e;
                        dv[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(pdt[e], gp[r][e], dv[cb], 0, 0, 0);
                        dk[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(dst[e], Qs[qq * LDT + l15], dk[cb], 0, 0, 0);
                    }
                }
                // dQ rows of block r: (queries 4*lg + e, channel l15)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int qq = r * 16 + lg * 4 + e;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dq[e] * a.q_scale), dq_rs, qq * (3 * D * 4) + dq_col, 0, 0);
                    sq += dq[e] * a.q_scale;   // rows >= T are exactly zero (their dS is masked)
                }
            }
            float sk = 0.f, sv = 0.f;
#pragma unroll
            for (int cb = 0; cb < RB; ++cb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int kk = cb * 16 + lg * 4 + e;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dk[cb][e] * a.q_scale), dq_rs, kk * (3 * D * 4) + D * 4 + dq_col, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dv[cb][e]), dq_rs, kk * (3 * D * 4) + 2 * D * 4 + dq_col, 0, 0);
                    sk += dk[cb][e] * a.q_scale;
                    sv += dv[cb][e];
                }
            sq = lg4_sum(sq);
            sk = lg4_sum(sk);
            sv = lg4_sum(sv);
            if (lg == 0) {
                float* lp = a.lnpart + (size_t)win * 6 * D + 3 * D + head * 16 + l15;
                lp[0] = sq;
                lp[D] = sk;
                lp[2 * D] = sv;
            }
            __builtin_amdgcn_wave_barrier();   // the scratch tiles are rewritten by the next head
        }
        bwd_stamp(a.trace, 12);
        __syncthreads();   // every head's dq | dk | dv rows of this window are in HBM/L2 (and visible to the other waves)
        bwd_stamp(a.trace, 13);
        // ---- dx_in = dz1 + dqkv [48 x 768] * Wqkv^T -------------------------------------------------------------------------------
        // The dq | dk | dv rows just written (L2) are staged through LDS in 6 chunks of 128 columns, double-buffered in the
        // per-wave scratch region (free by now): coalesced 512-byte row segments once per workgroup instead of every wave
        // gathering 64-byte pieces of all 48 rows per k-block (that form ran this product at 55 % of its MFMA time).
        {
            constexpr int KC = 128, LDA = 136, NCH = 3 * D / KC;
            static_assert(2 * RP * LDA <= 8 * 3 * RP * 20, "chunk buffers fit the scratch region");
            // hybrid row tiling (fused_encoder_h_kernel): rows 0-31 on 16x16x4, rows 32-39 on 4x4x1 MFMAs, nothing on the pad rows
            using namespace fzh;
            // The accumulators START at dz1 (the residual path of dx_in = dz1 + dqkv Wqkv^T) instead of at zero, so that the epilogue
            // only stores: written as `dx_in[i] = dz1[i] + acc` per element it compiled to one dependent load -> wait -> store round
            // trip per element, 20 per lane at the end of every window (the optimiser may not move a load across a store it cannot
            // prove disjoint, tip_pgemm.h), and this kernel has no registers left to batch the loads in.  Tail blocks: lane group 0
            // carries dz1 in its k-partial, the other three start at zero (tail_reduce sums the four).
            f32x4 acc_i[RBM][2], acc_it[RBT][2];
            const __amdgpu_buffer_rsrc_t z_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dz1) + grow0 * D, 0, T * D * 4, 0x00020000);
            const __amdgpu_buffer_rsrc_t x_rs = __builtin_amdgcn_make_buffer_rsrc(a.dx_in + grow0 * D, 0, T * D * 4, 0x00020000);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int col = (wave * 2 + n) * 16 + l15;
#pragma unroll
                for (int r = 0; r < RBM; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int row = r * 16 + lg * 4 + e;      // rows >= T: outside the buffer -> 0
                        acc_i[r][n][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(z_rs, (row * D + col) * 4, 0, 0));
                    }
#pragma unroll
                for (int rb = 0; rb < RBT; ++rb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int row = TAIL0 + 4 * rb + e;
                        const float zv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(z_rs, (row * D + col) * 4, 0, 0));
                        acc_it[rb][n][e] = lg == 0 ? zv : 0.f;
                    }
            }
            float* Ab = Sc;
            const int wq = lbase + (int)(fb::WQT * 4) + (wave * 2) * 48 * 1024;
            WRing<2> g_q;
            ring_prefetch<2>(g_q, rsrc, voff, wq, 48 * 1024);
            f32x4 st[3];   // this thread's 3 float4 of a chunk: element i = tid + 512 j -> row i / 32, columns 4 (i % 32) ..
            auto fetch = [&](int ch) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int i = tid + THREADS * j, row = i >> 5, c4 = i & 31;
                    st[j] = zero4;
                    if (row < T) st[j] = *reinterpret_cast<const f32x4*>(a.dqkv + (grow0 + row) * (3 * D) + ch * KC + c4 * 4);
                }
            };
            auto stash = [&](float* buf) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int i = tid + THREADS * j, row = i >> 5, c4 = i & 31;
                    *reinterpret_cast<f32x4*>(buf + row * LDA + c4 * 4) = st[j];
                }
            };
            fetch(0);
            stash(Ab);
            __syncthreads();
#pragma unroll 1
            for (int ch = 0; ch < NCH; ++ch) {
                if (ch + 1 < NCH) fetch(ch + 1);           // in flight during this chunk's MFMAs
                const int nx = ch + 1 < NCH ? wq + (ch + 1) * (KC / 16) * 1024 : wq;
                const float* Ac = Ab + (ch & 1) * RP * LDA;
                gemm_phase_h<2, KC / 16, 0, true>(acc_i, acc_it, Ac + l15 * LDA + lg * 4, Ac + (TAIL0 + (lane & 3)) * LDA + lg * 4, LDA, rsrc, voff,
                                                  wq + ch * (KC / 16) * 1024, 48 * 1024, g_q, nx, 48 * 1024);
                if (ch + 1 < NCH) stash(Ab + ((ch + 1) & 1) * RP * LDA);
                __syncthreads();
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int col = (wave * 2 + n) * 16 + l15;
#pragma unroll
                for (int r = 0; r < RBM; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int row = r * 16 + lg * 4 + e;
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc_i[r][n][e]), x_rs, (row * D + col) * 4, 0, 0);
                    }
#pragma unroll
                for (int rb = 0; rb < RBT; ++rb) {
                    const int row = TAIL0 + 4 * rb + lg;
                    const float v = tail_reduce(acc_it[rb][n], lg);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), x_rs, (row * D + col) * 4, 0, 0);
                }
            }
        }
        bwd_stamp(a.trace, 14);
        __syncthreads();
    }
}

hipError_t launch_attn_bwd(const Dims& d, const AttnBwdArgs& a, int B, int T, int num_cus, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (!fused_supported(d, T)) return hipErrorInvalidValue;
    constexpr int lds = (fz::RP * fz::LDX + 8 * 3 * fz::RP * 20) * 4;   // datt_o + per-wave Q / K / dO transposition tiles
    static_assert(8 * 3 * fz::RP * 20 >= 8 * 3 * fz::D, "the LayerNorm partial scratch lives in the per-wave scratch region");
    if ((long long)B * T * 3 * d.D * 4 > 0x7fffffffLL) return hipErrorInvalidValue;
    if (hipError_t e = dynamic_lds<attn_bwd_kernel<false>, attn_bwd_kernel<true>>(lds)) return e;
    AttnBwdArgs aa = a;
    aa.dqkv_bytes = (int)((long long)B * T * 3 * d.D * 4);
    aa.trace = measure_switches().bwd_trace ? 1 : 0;
    if (aa.thresh) hipLaunchKernelGGL(attn_bwd_kernel<true>, dim3(B < num_cus ? B : num_cus), dim3(fz::THREADS), lds, s, aa, B, T);
    else hipLaunchKernelGGL(attn_bwd_kernel<false>, dim3(B < num_cus ? B : num_cus), dim3(fz::THREADS), lds, s, aa, B, T);
    return hipGetLastError();
}

// =====================================================================================================================
// Training step, the dX products outside the encoder layers, per window:  out[T][N] = A[T][K] W'^T  with W' [N][16 KB] in
// fragment order.  These were batch-wide LDS-tiled GEMMs (tgemm16: dH = dy W_out 29.7 us, d_enc = delta W_ih 36.6 us at B = 256 —
// 46 / 73 TFLOP/s: 10 240 rows x 256-512 columns is 640-1 280 tiles of 64 x 64 on 256 CUs with both operands staged per tile);
// here a workgroup takes one window: its 40 rows go to LDS once (whole K), each wave owns NBW column blocks and streams their
// weight fragments through the register ring of the fused kernels, rows 0-31 on 16x16x4 and rows 32-39 on 4x4x1 MFMAs
// (gemm_phase_h) — nothing on pad rows, no per-tile operand staging.
//   <2, 32>: N = 256, K = 512 (d_enc);   <4, 10>: N = 512, K = 160 (dH: dy padded to 144 columns, the k-blocks come in pairs)
// =====================================================================================================================
template <int NBW, int KB>
__global__ __launch_bounds__(fz::THREADS) void win_gemm_kernel(WinGemmArgs a, int B, int T) {
    using namespace fz;
    using namespace fzh;
    constexpr int K = KB * 16, LDA = K + 8, C4 = K / 4, NI = (RP * C4 + THREADS - 1) / THREADS;
    extern __shared__ __attribute__((aligned(16))) float smem[];   // A rows [RP][LDA]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wfrag), 0, a.wbytes, 0x00020000);
    const int voff = lane * 16;
    const int wsoff = wave * NBW * KB * 1024;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    for (int win = blockIdx.x; win < B; win += gridDim.x) {
        WRing<NBW> g;
        ring_prefetch<NBW>(g, rsrc, voff, wsoff, KB * 1024);
        // the window's rows -> LDS: every load in flight before the first store (clamped addresses, zeros afterwards)
        f32x4 v[NI];
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int i = tid + j * THREADS, row = i / C4, c = (i - row * C4) * 4;
            const int rc = row < T ? row : T - 1, cc = c < a.kvalid ? c : a.kvalid - 4;
            v[j] = *reinterpret_cast<const f32x4*>(a.A + ((size_t)win * T + rc) * a.lda + cc);
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int i = tid + j * THREADS, row = i / C4, c = (i - row * C4) * 4;
            if (i < RP * C4) *reinterpret_cast<f32x4*>(smem + row * LDA + c) = (row < T && c < a.kvalid) ? v[j] : zero4;
        }
        __syncthreads();
        f32x4 acc[RBM][NBW], acct[RBT][NBW];
        zero_acc_h<NBW>(acc, acct);
        // rows 0-31 with swapped operands (transposed accumulators: lane = row l15, columns 4 lg ..): one 16-byte store per tile instead
        // of four 4-byte ones; the window's output rows as a buffer of T rows, so the pad rows are dropped by the range check instead
        // of by a branch around every store (as the hybrid encoder's IH epilogue).  Same products, same sums.
        gemm_phase_h<NBW, KB, NBW, true>(acc, acct, smem + l15 * LDA + lg * 4, smem + (TAIL0 + (lane & 3)) * LDA + lg * 4, LDA, rsrc, voff, wsoff,
                                         KB * 1024, g, wsoff, KB * 1024);
        const __amdgpu_buffer_rsrc_t o_rs = tip_rows_buffer(a.out + (size_t)win * T * a.ldo, T * a.ldo * 4);
#pragma unroll
        for (int n = 0; n < NBW; ++n) {
#pragma unroll
            for (int r = 0; r < RBM; ++r)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[r][n]), o_rs,
                                                       ((r * 16 + l15) * a.ldo + (wave * NBW + n) * 16 + lg * 4) * 4, 0, 0);
#pragma unroll
            for (int rb = 0; rb < RBT; ++rb)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(tail_reduce(acct[rb][n], lg)), o_rs,
                                                      ((TAIL0 + 4 * rb + lg) * a.ldo + (wave * NBW + n) * 16 + l15) * 4, 0, 0);
        }
        __syncthreads();   // the next window's rows overwrite the LDS image
    }
}

template <int NBW, int KB>
static hipError_t launch_win_gemm_t(const WinGemmArgs& a, int B, int T, int num_cus, hipStream_t s) {
    constexpr int lds = fz::RP * (KB * 16 + 8) * 4;
    if (hipError_t e = dynamic_lds<win_gemm_kernel<NBW, KB>>(lds)) return e;
    hipLaunchKernelGGL((win_gemm_kernel<NBW, KB>), dim3(B < num_cus ? B : num_cus), dim3(fz::THREADS), lds, s, a, B, T);
    return hipGetLastError();
}

// N = 16 * 8 * nbw columns, K = 16 * kb (weights [N][K] in fragment order, zero padded); hipErrorInvalidValue for other shapes
hipError_t launch_win_gemm(int N, int K, const WinGemmArgs& a, int B, int T, int num_cus, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (T < 1 || T > fz::TMAX || a.kvalid % 4 || a.kvalid < 4 || a.kvalid > K || a.lda % 4 || a.ldo % 4 || (reinterpret_cast<uintptr_t>(a.out) & 15) || (long long)T * a.ldo * 4 > 0x7fffffffLL || (long long)N * K * 4 != (long long)a.wbytes)
        return hipErrorInvalidValue;
    if (N == 256 && K == 512) return launch_win_gemm_t<2, 32>(a, B, T, num_cus, s);
    if (N == 512 && K == 160) return launch_win_gemm_t<4, 10>(a, B, T, num_cus, s);
    return hipErrorInvalidValue;
}

}  // namespace tip

extern "C" int tip_debug_read_bwd_trace(unsigned long long* out, int n) {
    if (!out || n < 0 || n > 16) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(tip::g_bwd_trace), sizeof(unsigned long long) * n) == hipSuccess ? 0 : -5;
}
