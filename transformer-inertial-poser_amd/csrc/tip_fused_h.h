// tip_fused_h.h — the device pieces of the fused plans and the WHOLE one-window hybrid encoder (fused_encoder_h_kernel) as a device
// function, shared by the stand-alone kernel (tip_fused.hip) and the one-launch round (forward_round_kernel, tip_round.hip).
#pragma once
#include "tip_internal.h"
#include "tip_attention.h"
#include "tip_layernorm.h"

namespace tip {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace fz {
constexpr int D = 256, H = 16, DH = 16, F = 1024, RP = 48, RB = 3, TMAX = 40, R = 512;
constexpr int KIN = 224;            // in_linear K, zero padded (221 with acc-sum, 203 without)
// Row strides of the A-operand planes are = 8 (mod 64) dwords, not the usual "+ 4".  An A fragment is one ds_read_b128 per lane: row
// l15, dwords 4 lg .. 4 lg + 3 of the k-block.  The LDS serves a b128 read in four groups of 16 lanes that are NOT contiguous —
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md, LDS) — i.e. rows {0-3, 12-15} at one k offset together with rows
// {4-11} at the NEXT k offset.  In units of 16-byte slots (16 per LDS line) lane (l15, lg) hits slot (s * l15 + lg) mod 16, s = stride / 4
// mod 16: with s = 1 (stride 260) the two row sets land on {0-3, 12-15} and {5-12} — slot 12 twice, every read 5 LDS cycles instead of
// 4; with s = 2 (stride 264) on the even and the odd slots.  SQ_LDS_BANK_CONFLICT of the hybrid encoder: 26.4 M -> 3.6 M cycles per
// launch (the tail fragments' four rows x two k offsets likewise: {0-3} and {1-4} -> {0, 2, 4, 6} and {1, 3, 5, 7}).
constexpr int LDX = D + 8;          // 264
constexpr int LDC = 128 + 4;        // 132: one Q / K plane of an 8-head chunk, [48 rows][128 channels]
constexpr int LDV = RP + 4;         // 52: V is kept TRANSPOSED, [128 channels][48 keys], so P.V reads B fragments as b128
constexpr int LDU = KIN + 8;        // 232
constexpr int X_FLOATS = RP * LDX;              // 12480
constexpr int C_FLOATS = 2 * RP * LDC + 128 * LDV;   // 19328
constexpr int LDS_BYTES = (X_FLOATS + C_FLOATS) * 4;
constexpr int THREADS = 512;
// packed section (floats)
constexpr size_t IN_W = 0;
constexpr size_t IN_B = IN_W + (size_t)D * KIN;
constexpr size_t LAYER0 = IN_B + D;
constexpr size_t QKV_W = 0;
constexpr size_t QKV_B = QKV_W + (size_t)3 * D * D;
constexpr size_t WO_W = QKV_B + 3 * D;
constexpr size_t WO_B = WO_W + (size_t)D * D;
constexpr size_t W1_W = WO_B + D;
constexpr size_t W1_B = W1_W + (size_t)F * D;
constexpr size_t W2_W = W1_B + F;
constexpr size_t W2_B = W2_W + (size_t)D * F;
constexpr size_t G1 = W2_B + D;
constexpr size_t BE1 = G1 + D;
constexpr size_t G2 = BE1 + D;
constexpr size_t BE2 = G2 + D;
constexpr size_t LAYER_FLOATS = BE2 + D;
constexpr size_t TAIL_PAD = 4096;      // the k-loop prefetches up to 2 blocks (2 KiB) past a wave's last block
}  // namespace fz

// ------------------------------------------------------------------------------------------------------------
// device pieces
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wsum(float v) { return wave64_sum(v); }   // DPP + permlane swaps, no LDS round trips

// acc[r][n] += A(rows of block r) x W(block n).  For the first SWAPN column blocks the MFMA operands are swapped (weights
// as A, activations as B): the accumulator then holds the TRANSPOSED tile — (channels 4*lg + e, row l15) — which is the
// fragment layout a following MFMA wants for Q and K (tip_attention.h, attention_head_regs).
template <int NBW, int SWAPN = 0>
__device__ __forceinline__ void mfma_block(f32x4 (&acc)[fz::RB][NBW], const float4 (&a)[fz::RB], const float4 (&w)[NBW]) {
#define TIP_MFMA_STEP(c)                                                                                             \
    _Pragma("unroll") for (int r = 0; r < fz::RB; ++r) _Pragma("unroll") for (int n = 0; n < NBW; ++n)                \
        acc[r][n] = n < SWAPN ? __builtin_amdgcn_mfma_f32_16x16x4f32(w[n].c, a[r].c, acc[r][n], 0, 0, 0)              \
                              : __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].c, w[n].c, acc[r][n], 0, 0, 0);
    TIP_MFMA_STEP(x)
    TIP_MFMA_STEP(y)
    TIP_MFMA_STEP(z)
    TIP_MFMA_STEP(w)
#undef TIP_MFMA_STEP
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// One 1-KiB fragment block: lane l gets bytes [16 l, 16 l + 16) of the block at byte offset `soff`.
// raw buffer loads (SGPR descriptor + scalar offset) instead of flat loads: the optimiser treats them as opaque
// calls, so the software-pipelined prefetch below survives (flat loads from __restrict__ memory were re-sunk to
// their use, exposing the L2 latency every k-step), and addresses cost one VGPR.
__device__ __forceinline__ float4 load_frag(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff) {
    // NB: bit-cast the whole vector — __builtin_bit_cast(float, v[i]) on a vector ELEMENT is miscompiled by this
    // clang (every element reads lane 0 of the vector).
    const f32x4 f = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0));
    return make_float4(f.x, f.y, f.z, f.w);
}

// Register ring of weight fragments: k-blocks (even, odd) of the NBW column blocks a wave owns.
template <int NBW>
struct WRing {
    float4 w0[NBW], w1[NBW];
};

// Prime a ring with k-blocks 0 and 1 of a phase.  Called EARLY (before the epilogue / barrier / LayerNorm /
// attention that precedes the phase) so the L2 latency of a phase's first fragments is never exposed.
template <int NBW>
__device__ __forceinline__ void ring_prefetch(WRing<NBW>& g, __amdgpu_buffer_rsrc_t rsrc, int voff, int soff, int nstride_b) {
#pragma unroll
    for (int n = 0; n < NBW; ++n) {
        g.w0[n] = load_frag(rsrc, voff, soff + n * nstride_b);
        g.w1[n] = load_frag(rsrc, voff, soff + n * nstride_b + 1024);
    }
}

// acc[r][n] += A[48 x 16*KB] (LDS, leading dim lda) * Wblock(n, kb)   for kb in [0, KB)
//   soff: byte offset (wave-uniform) of the wave's first block at kb = 0; block n is + n*nstride_b; k-block kb is + kb*1024.
//   The ring holds k-blocks 0,1 on entry.  The prefetch runs two k-blocks ahead and is unconditional (branch-free
//   loop => counted vmcnt waits); for the LAST pair it is redirected to k-blocks 0,1 of the NEXT phase
//   (nsoff / nnstride_b), so on exit the ring is already primed for a following phase of the same width.
//   Callers without such a successor pass their own soff (a harmless in-bounds reload).
template <int NBW, int KB, int SWAPN = 0, bool PIN = true>
__device__ __forceinline__ void gemm_phase(f32x4 (&acc)[fz::RB][NBW], const float* As, int lda, __amdgpu_buffer_rsrc_t rsrc,
                                           int voff, int soff, int nstride_b, WRing<NBW>& g, int nsoff, int nnstride_b) {
    static_assert(KB % 2 == 0, "k-blocks are processed in pairs");
    // A fragments are double-buffered too: the ds_read_b128 of k-block kb+1 is in flight while the MFMAs of kb issue.
    // (Reads past the last k-block stay inside the LDS allocation and are never used.)
    float4 a0[fz::RB], a1[fz::RB];
#pragma unroll
    for (int r = 0; r < fz::RB; ++r) a0[r] = *reinterpret_cast<const float4*>(As + r * 16 * lda);
#pragma unroll 1
    for (int kb = 0; kb < KB; kb += 2) {
        const bool last = kb + 2 >= KB;                       // wave-uniform: scalar selects, no branch
        const int o = last ? nsoff : soff + (kb + 2) * 1024;
        const int st = last ? nnstride_b : nstride_b;
#pragma unroll
        for (int r = 0; r < fz::RB; ++r) a1[r] = *reinterpret_cast<const float4*>(As + r * 16 * lda + (kb + 1) * 16);
        mfma_block<NBW, SWAPN>(acc, a0, g.w0);
#pragma unroll
        for (int n = 0; n < NBW; ++n) g.w0[n] = load_frag(rsrc, voff, o + n * st);
        // PIN: keep the refill here (the scheduler may sink it towards its use).  Measured: helps the training forward and the
        // backward kernels by ~1 %, costs the stash-free inference kernel 0.7 % — which therefore opts out
        if (PIN) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < fz::RB; ++r) a0[r] = *reinterpret_cast<const float4*>(As + r * 16 * lda + (kb + 2) * 16);
        mfma_block<NBW, SWAPN>(acc, a1, g.w1);
#pragma unroll
        for (int n = 0; n < NBW; ++n) g.w1[n] = load_frag(rsrc, voff, o + n * st + 1024);
        if (PIN) __builtin_amdgcn_sched_barrier(0);
    }
}

template <int NBW>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[fz::RB][NBW]) {
#pragma unroll
    for (int r = 0; r < fz::RB; ++r)
#pragma unroll
        for (int n = 0; n < NBW; ++n) acc[r][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// LayerNorm of the residual stream: tip_layernorm.h (16 lanes per row, DPP reductions), all 48 rows here — the pad rows of the
// padded kernels evolve like real ones and must stay finite.
// The training forward's stash stores have per-thread row / column offsets that are loop invariant; hoisted out of the layer
// loop they cost ~50 VGPRs for the whole kernel (hundreds of bytes of scratch per lane).  An opaque copy of the thread index at
// each use keeps them where they are consumed: a dozen VALU instructions per store loop.
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// rows 0..T-1 of an LDS tile [rows][ld] (COLS floats wide) -> HBM rows of stride dst_ld, 16-byte streaming stores (the stash, 2 MB per
// window, is read next by the backward; the weights it would push out of L2 in 0.1 us), with a FIXED number of stores per thread
// (T <= 40: the hybrid kernel), rows >= T dropped by the buffer's range check instead of by a loop bound.  With a run-time trip count
// the compiler cannot count the stores in flight, and the `s_waitcnt vmcnt(N)`
// of the weight ring behind such a loop (vector memory retires in order, stores included) degenerates to "all but the last few":
// every stash point waited for its own stores' acknowledgement before the next phase's first MFMA.
template <int COLS>
__device__ __forceinline__ void rows_to_hbm_fixed(const float* lds, int ld, float* dst, int dst_ld, int T, int tid) {
    constexpr int C4 = COLS / 4, NP = (40 * C4 + fz::THREADS - 1) / fz::THREADS;
    static_assert((NP * fz::THREADS + C4 - 1) / C4 <= fz::RP, "the passes stay inside the LDS tile's rows");
    const __amdgpu_buffer_rsrc_t rs = tip_rows_buffer(dst, T * dst_ld * 4);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int i = tid + j * fz::THREADS, r = i / C4, c4 = i - r * C4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(lds + r * ld + c4 * 4);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ln_u32x4, v), rs, (r * dst_ld + c4 * 4) * 4, 0, kTipNT);
    }
}

// The training forward's hidden chunk [T][256] (after ReLU and dropout): rows to HBM as rows_to_hbm_fixed does, plus the chunk's gates
// (hidden > 0) as BITS for the fused FFN backward.  gb points at row 0 of the window in the gate-bit array [M][32 dwords]:
//   dword (row, f*8 + 2*e + (c4 >> 5)), bit (c4 & 31)  =  hidden[row][f*256 + 4*c4 + e] > 0      (c4 = 0..63: column quad)
// One wave iteration is one row (64 lanes = its 64 column quads): four ballots, 32 bytes stored by lane 0.  Round 5: ffn_bwd_kernel
// read the gates as the saved fp32 hidden rows — 42 MB per layer that arrive cold from HBM in front of each chunk's weight ring
// (vector memory returns in order: every chunk stalled ~4 000 cycles behind them); as bits they are 1.3 MB, staged into LDS once per window.
// Five stores per thread whatever T <= 40 is (as rows_to_hbm_fixed); lanes other than 0 drop the bit stores.
__device__ __forceinline__ void hidden_to_hbm(const float* lds, int ld, float* dst, int dst_ld, unsigned* gb, int f, int T, int tid) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const int lane = tid & 63;
    const __amdgpu_buffer_rsrc_t rs = tip_rows_buffer(dst, T * dst_ld * 4);
    const __amdgpu_buffer_rsrc_t gs = tip_rows_buffer(reinterpret_cast<const float*>(gb), T * 128);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int r = (tid >> 6) + 8 * j;
        const f32x4 v = *reinterpret_cast<const f32x4*>(lds + r * ld + lane * 4);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ln_u32x4, v), rs, (r * dst_ld + lane * 4) * 4, 0, kTipNT);
        const unsigned long long b0 = __builtin_amdgcn_ballot_w64(v[0] > 0.f), b1 = __builtin_amdgcn_ballot_w64(v[1] > 0.f);
        const unsigned long long b2 = __builtin_amdgcn_ballot_w64(v[2] > 0.f), b3 = __builtin_amdgcn_ballot_w64(v[3] > 0.f);
        const int off = lane == 0 ? r * 128 + f * 32 : 0x7fffff00;      // one lane writes the row's 32 bytes; the others fall outside the buffer
        const u32x4 lo = {(unsigned)b0, (unsigned)(b0 >> 32), (unsigned)b1, (unsigned)(b1 >> 32)};
        const u32x4 hi = {(unsigned)b2, (unsigned)(b2 >> 32), (unsigned)b3, (unsigned)(b3 >> 32)};
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ln_u32x4, lo), gs, off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ln_u32x4, hi), gs, off, 16, 0);
    }
}

// =====================================================================================================================
// "fusedh": the one-window kernel with a HYBRID row tiling — no matrix-core work on padded rows.
//
// T = 40 rows do not fill three 16-row MFMA blocks: in fused_encoder_kernel every weight fragment multiplies rows 0-15,
// 16-31 and 32-47, and a third of that last block's cycles (17 % of all MFMA issue time) is spent on the eight zero rows
// 40-47.  Here rows 0-31 keep v_mfma_f32_16x16x4_f32 (two row blocks), and rows 32-39 go through
// v_mfma_f32_4x4x1_16b_f32 — sixteen independent 4x4x1 blocks per instruction, 512 FLOP in 2 passes (measured 8.4-9 cycles
// per instruction against 32 for a 16x16x4: tools/probes/mfma4x4_probe.hip) — fed by THE SAME B-fragment registers:
//   the 16x16x4 weight fragment has lane (l15, lg) = W[col 16 nb + l15][k = 16 kb + 4 lg + s] in component s.  Read as the
//   B operand of a 4x4x1, lane 4 b + j is column j of block b: block b = 4 lg + (l15 >> 2), j = l15 & 3, i.e. block
//   (lg, cb) multiplies columns 4 cb .. 4 cb + 3 at k = 16 kb + 4 lg + s.  Its A operand (lane 4 b + i = row i of block b)
//   is X[row0 + i][16 kb + 4 lg + s]: one ds_read_b128 per (4-row block, k-block), lanes that differ only in cb reading the
//   same address (LDS broadcast).  The accumulator of lane (lg, cb, j) then holds, in register i, the partial sum over the
//   k == 4 lg .. 4 lg + 3 (mod 16) of output (row0 + i, column 16 nb + 4 cb + j): four k-partials per output, one per lg,
//   combined once per phase by a two-step exchange (xor 32, xor 16) that leaves row row0 + lg in lane (lg, l15).
// Per (16-column block, k-block): 8 big + 8 small MFMAs = 8 x 32 + 8 x 9 = 328 issue cycles instead of 12 x 32 = 384.
// The QKV projection does the same; its rows 32..39 reach the attention's register fragments (attention_head_regs: Q^T / K^T
// tiles with the row in the lane index) through a 1.3-KB per-wave LDS patch that transposes the tail's (row, channel) result.
// Rows 40-47 of X are zeroed once and never written again (LayerNorm covers rows 0-39): finite pad keys/values for the attention.
// Numerics: rows 0-31 are bit-identical to TIP_PLAN_FUSED (same instructions; causality keeps rows >= 32 out of them);
// rows 32-39 differ in summation order only (four k-chains per output instead of one).
// =====================================================================================================================
namespace fzh {
constexpr int RBM = 2;    // 16-row MFMA blocks (rows 0-31)
constexpr int RBT = 2;    // 4-row blocks of the tail (rows 32-35, 36-39)
constexpr int TAIL0 = 32;
}  // namespace fzh

// (the first SWAPN column blocks of the 16-row part with swapped operands, as in mfma_block: transposed accumulators)
template <int NBW, int SWAPN = 0>
__device__ __forceinline__ void mfma_block_h(f32x4 (&acc)[fzh::RBM][NBW], f32x4 (&acct)[fzh::RBT][NBW], const float4 (&a)[fzh::RBM],
                                             const float4 (&at)[fzh::RBT], const float4 (&w)[NBW]) {
#define TIP_MFMA_STEP_H(c)                                                                                            \
    _Pragma("unroll") for (int r = 0; r < fzh::RBM; ++r) _Pragma("unroll") for (int n = 0; n < NBW; ++n)               \
        acc[r][n] = n < SWAPN ? __builtin_amdgcn_mfma_f32_16x16x4f32(w[n].c, a[r].c, acc[r][n], 0, 0, 0)              \
                              : __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].c, w[n].c, acc[r][n], 0, 0, 0);             \
    _Pragma("unroll") for (int r = 0; r < fzh::RBT; ++r) _Pragma("unroll") for (int n = 0; n < NBW; ++n)               \
        acct[r][n] = __builtin_amdgcn_mfma_f32_4x4x1f32(at[r].c, w[n].c, acct[r][n], 0, 0, 0);
    TIP_MFMA_STEP_H(x)
    TIP_MFMA_STEP_H(y)
    TIP_MFMA_STEP_H(z)
    TIP_MFMA_STEP_H(w)
#undef TIP_MFMA_STEP_H
}

// acc  [r][n] += A[rows 16 r .. 16 r + 15] x Wblock(n, kb)      (r = 0, 1)
// acct [r][n] += A[rows 32 + 4 r .. + 3]  x Wblock(n, kb), per-lg k-partials (see above)
//   Am: this lane's LDS address for the 16-row blocks (base + l15 * lda + lg * 4);  At: for the tail (base + (32 + (lane & 3)) *
//   lda + lg * 4).  Weight ring semantics exactly as gemm_phase.
template <int NBW, int KB, int SWAPN = 0, bool PIN = false>
__device__ __forceinline__ void gemm_phase_h(f32x4 (&acc)[fzh::RBM][NBW], f32x4 (&acct)[fzh::RBT][NBW], const float* Am, const float* At,
                                             int lda, __amdgpu_buffer_rsrc_t rsrc, int voff, int soff, int nstride_b, WRing<NBW>& g,
                                             int nsoff, int nnstride_b) {
    static_assert(KB % 2 == 0, "k-blocks are processed in pairs");
    float4 a0[fzh::RBM], a1[fzh::RBM], t0[fzh::RBT], t1[fzh::RBT];
#pragma unroll
    for (int r = 0; r < fzh::RBM; ++r) a0[r] = *reinterpret_cast<const float4*>(Am + r * 16 * lda);
#pragma unroll
    for (int r = 0; r < fzh::RBT; ++r) t0[r] = *reinterpret_cast<const float4*>(At + r * 4 * lda);
#pragma unroll 1
    for (int kb = 0; kb < KB; kb += 2) {
        const bool last = kb + 2 >= KB;
        const int o = last ? nsoff : soff + (kb + 2) * 1024;
        const int st = last ? nnstride_b : nstride_b;
#pragma unroll
        for (int r = 0; r < fzh::RBM; ++r) a1[r] = *reinterpret_cast<const float4*>(Am + r * 16 * lda + (kb + 1) * 16);
#pragma unroll
        for (int r = 0; r < fzh::RBT; ++r) t1[r] = *reinterpret_cast<const float4*>(At + r * 4 * lda + (kb + 1) * 16);
        mfma_block_h<NBW, SWAPN>(acc, acct, a0, t0, g.w0);
#pragma unroll
        for (int n = 0; n < NBW; ++n) g.w0[n] = load_frag(rsrc, voff, o + n * st);
        if (PIN) __builtin_amdgcn_sched_barrier(0);   // (as in gemm_phase: keeps the refill ahead of the second half's MFMAs)
#pragma unroll
        for (int r = 0; r < fzh::RBM; ++r) a0[r] = *reinterpret_cast<const float4*>(Am + r * 16 * lda + (kb + 2) * 16);
#pragma unroll
        for (int r = 0; r < fzh::RBT; ++r) t0[r] = *reinterpret_cast<const float4*>(At + r * 4 * lda + (kb + 2) * 16);
        // the NEXT pair's first A fragments are requested HERE, half an iteration ahead: left to itself the scheduler sinks these reads
        // to the top of the next iteration, right in front of the MFMA that needs them, and both waves of a SIMD — in step behind every
        // barrier — then sit out an LDS round trip per k-block pair with the matrix pipe idle
        __builtin_amdgcn_sched_barrier(0);
        mfma_block_h<NBW, SWAPN>(acc, acct, a1, t1, g.w1);
#pragma unroll
        for (int n = 0; n < NBW; ++n) g.w1[n] = load_frag(rsrc, voff, o + n * st + 1024);
        if (PIN) __builtin_amdgcn_sched_barrier(0);
    }
}

template <int NBW>
__device__ __forceinline__ void zero_acc_h(f32x4 (&acc)[fzh::RBM][NBW], f32x4 (&acct)[fzh::RBT][NBW]) {
#pragma unroll
    for (int n = 0; n < NBW; ++n) {
#pragma unroll
        for (int r = 0; r < fzh::RBM; ++r) acc[r][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < fzh::RBT; ++r) acct[r][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
}

// Combine the four k-partials of a tail accumulator (registers = rows row0 .. row0 + 3, one partial per lg): two exchange
// steps, after which lane (lg, l15) holds the finished sum of row row0 + lg, column l15 of the block.  Every row is summed
// as (p[lg] + p[lg ^ 2]) + (p[lg ^ 1] + p[lg ^ 3]) — the same pairing for all four rows.
// Three permlane swaps (tip_layernorm.h), no LDS crossbar: swap32(v0, v2) leaves {v0.lo, v2.lo} and {v0.hi, v2.hi}, whose sum is
// row 0 in lanes 0-31 and row 2 in lanes 32-63 — exactly what "keep one row, hand the other to lane ^ 32" produces.
__device__ __forceinline__ float tail_reduce(const f32x4& v, int lg) {
    (void)lg;
    float a = v[0], b = v[2];
    swap32(a, b);
    float k0 = a + b;              // rows {0,1} live on with lg in {0,1}, rows {2,3} with lg in {2,3}
    a = v[1], b = v[3];
    swap32(a, b);
    float k1 = a + b;
    swap16(k0, k1);
    return k0 + k1;                // row 2 * (lg >> 1) + (lg & 1) = lg
}

// The V tile of rows 32..47 in the plain accumulator layout (lane (l15, lg) = rows 32 + 4 lg + e, channel l15) from the two tail
// accumulators (a0: rows 32..35, a1: rows 36..39; four k-partials each, one per lg): all four rows of block lg must end up in
// ONE lane — an all-reduce over lg rather than tail_reduce's reduce-scatter.  swap16(a0, a1) pairs lg with lg ^ 1 and parks
// block 0 in the even, block 1 in the odd lane groups; swap32 of the sums finishes both.  Lanes lg = 2, 3 (pad rows 40..47,
// multiplied by P = 0 in the attention) get zeros.
__device__ __forceinline__ f32x4 tail_gather_v(const f32x4& a0, const f32x4& a1, int lg) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float x = a0[e], y = a1[e];
        swap16(x, y);
        float s = x + y, t = s;
        swap32(s, t);
        o[e] = s + t;
    }
    return lg < 2 ? o : (f32x4){0.f, 0.f, 0.f, 0.f};
}

// measurement only (TIP_FUSEDH_TRACE=1): s_memtime stamps of workgroup 0 / thread 0 at the phase boundaries of layer 1
// (defined in tip_fused.hip; only the TRACE instantiations, which live there, touch them)
extern __device__ unsigned long long g_fh_trace[64];
extern __device__ unsigned long long g_fh_wg[2 * 1024];   // TRACE: [workgroup][entry, exit] in s_memrealtime ticks (100 MHz, device-wide)
#define FH_STAMP(slot) do { if (TRACE && blockIdx.x == 0 && tid == 0 && (layer == 1 || (slot) < 4 || (slot) >= 40)) g_fh_trace[slot] = __builtin_amdgcn_s_memtime(); } while (0)

// Which windows a workgroup takes, and what it does once a window's outputs are stored.  FhGridStride is the stand-alone kernel's:
// windows blockIdx.x, + gridDim.x, ..., plain stores, nothing to publish (the kernel boundary does that).  The one-launch round
// (tip_round.hip) has a control of its own: one window, its IH rows and sentinel words stored write-through (kAux = 16, sc1: other
// XCDs read them inside the same launch) and a flag word behind them.  (A functor, not two integers: see HdGridStride, tip_head.h.)
struct FhGridStride {
    static constexpr int kAux = 0;   // cache policy of the IH / sentinel stores
    __device__ __forceinline__ int first() const { return blockIdx.x; }
    __device__ __forceinline__ int stride() const { return gridDim.x; }
    __device__ __forceinline__ void published(int, int) const {}
};

// The whole kernel as a device function.
// TR: training forward (tip_train_forward) — the encoder's four dropout sites and the activation stash of the backward, exactly
// as fused_encoder_kernel<8> writes them (same arrays, same per-element dropout keys: the masks do not depend on the tiling).
template <bool TRACE, bool TR, bool LIVE, class Ctl>
__device__ __forceinline__ void fused_encoder_h_body(
    const float* __restrict__ wts, const float* __restrict__ x_imu, const float* __restrict__ x_s, const float* __restrict__ keep_mask, float keep_scale, float* __restrict__ xout, float* __restrict__ ih_out,
    unsigned* __restrict__ hall_sentinel, int B, int T, int NI, int S, int L, int wbytes, int ih_off_b, const FusedEncArgs<LIVE>& tr, Ctl ctl) {
    // The statements are a file of their own because the stand-alone kernels include them DIRECTLY (tip_fused.hip): called through
    // this function, the same statements come out with another scalar register allocation (compared with tools/isa_diff.py), and
    // those kernels' code is what every figure of the plan was measured on.  One text, two ways into it.
#include "tip_fused_h_body.inc"
}

}  // namespace tip
