// tip_head.hip — output projection y = h W_out^T + b (/root/reference/simple_transformer_with_state.py:102) with the weight
// RESIDENT IN REGISTERS.
//
// N = 131 columns (9 blocks of 16), K = rnn_hidden = 512.  head_gemm_kernel (tip_general.hip) gives every wave 16 rows x 3
// column blocks and lets it stream its 98 KB of weight fragments from L2: 1 920 waves at B = 256 pull 190 MB through the
// CUs' vector L1s for a 1.4-GFLOP product, three passes over HALL (grid.y = 3) — 19.7 us, the matrix pipe 34 % busy.
//
// Here a workgroup is 8 waves that split K: wave w keeps k-blocks 4 w .. 4 w + 3 of ALL nine column blocks — 36 fragments,
// 144 VGPRs, loaded once — and the workgroup walks over row groups, reading every row of HALL exactly once (each wave its own
// 64-float slice of the row, straight into MFMA A fragments: no LDS staging of the operand).  The eight k-partials of a tile
// meet in LDS: every wave writes its accumulators in fragment order (conflict-free 16-byte writes), one barrier, and wave w
// sums column block w of all eight partials in a fixed order, adds the bias and stores.  The partial buffers alternate, so the
// only synchronisation is that one barrier per tile, and the reduction of tile i runs under the MFMAs of tile i + 1.
//
// Row tiling.  A window is T = 40 rows = two 16-row tiles (v_mfma_f32_16x16x4_f32) + 8 rows, and 256 windows on 256 CUs leave
// no room for a third padded tile per CU: rows 32-39 go through v_mfma_f32_4x4x1_16b_f32 fed by THE SAME weight registers (the
// hybrid row tiling of fused_encoder_h_kernel, tip_fused.hip): lane (l15, lg) of a 16x16x4 B fragment is column l15 at
// k = 16 kb + 4 lg + s, i.e. block (lg, l15 >> 2) / column l15 & 3 of a 4x4x1 whose A operand is h[row lane & 3] at the same k;
// the accumulator holds one k-partial per lg, combined by three permlane swaps.  Per window and SIMD: 2 x 9 216 + 2 x 2 592
// MFMA issue cycles instead of 3 x 9 216.
//   MODE 0  groups of 40 rows: tiles B(0) B(16) T(32) T(36)    — full output, T a multiple of 40 (a group never straddles windows)
//   MODE 2  groups of 4 rows:  tile T(0)                       — last-row output of the same windows
// A row's summation order depends on the tile kind only (B: per wave one MFMA chain over its 16 k-steps; T: four chains, one
// per lg, combined (p0 + p2) + (p1 + p3); then the eight waves ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7))).  In MODE 0 row
// t of a window is a T row iff t mod 40 >= 32, so row T - 1 always is: MODE 2 reproduces it bit for bit (forward_last ==
// forward[:, -1], tested).  Other window lengths, and state widths outside 129 .. 131, keep head_gemm_kernel in both forms.
#include "tip_head.h"

namespace tip {

__device__ unsigned long long g_hd_trace[32];
__device__ unsigned long long g_hd_wg[2 * 1024];   // [wg][entry, exit] in s_memrealtime ticks (100 MHz, device-wide counter)

template <int MODE, bool TRACE = false>
__global__ __launch_bounds__(hd::THREADS) void head_ksplit_kernel(const float* __restrict__ A, unsigned lda_b, unsigned a_bytes,
                                                                  const float* __restrict__ wfrag, const float* __restrict__ bias,
                                                                  float* __restrict__ Y, int ldy, int M, int N, int ngroups) {
    head_ksplit_body<MODE, TRACE, 0>(A, lda_b, a_bytes, wfrag, bias, Y, ldy, M, N, ngroups, HdGridStride{});
}

// tip_forward_rows: one output row per window, row rows[m] of window m (HdGather).  MODE 1 (B-tile rows) first looks whether any
// window of its groups wants a B-tile row and leaves at once when none does — a stream past its warm-up asks for row 39 only.
template <int MODE>
__global__ __launch_bounds__(hd::THREADS) void head_rows_kernel(const float* __restrict__ A, unsigned a_bytes,
                                                                const float* __restrict__ wfrag, const float* __restrict__ bias,
                                                                float* __restrict__ Y, int ldy, int M, int N, int ngroups, HdGather rsel) {
    if (MODE == 1) {
        int any = 0;
        if (threadIdx.x < 16)
            for (int g = blockIdx.x; g < ngroups; g += gridDim.x) any |= rsel.code(g * 16 + (int)threadIdx.x) == 1;
        if (!__syncthreads_or(any)) return;
    }
    head_ksplit_body<MODE, false, 0>(A, rsel.ld_b, a_bytes, wfrag, bias, Y, ldy, M, N, ngroups, HdGridStride{}, rsel);
}

extern "C" int tip_debug_read_head_wg(unsigned long long* out, int n) {
    if (!out || n < 0 || n > 2048) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hd_wg), sizeof(unsigned long long) * n) == hipSuccess ? 0 : -5;
}

extern "C" int tip_debug_read_head_trace(unsigned long long* out, int n) {
    if (!out || n < 0 || n > 32) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hd_trace), sizeof(unsigned long long) * n) == hipSuccess ? 0 : -5;
}

// Y[M, N] = A[M, 512] W^T + b on the register-resident kernel above.  rows_per_window: T (a multiple of 40) for the full output,
// ignored for last_only (M = one row per window).  Returns hipErrorInvalidValue for shapes it does not serve (the caller then
// keeps head_gemm_kernel).
hipError_t launch_head_ksplit(const float* A, long long lda, const float* wfrag, const float* bias, float* Y, int ldy, int M, int N,
                              int K, bool last_only, int num_cus, hipStream_t s, const int* rows, int rows_T) {
    if (M <= 0) return hipSuccess;
    // Column block 8 keeps THREE columns (128 .. 130) in its compact image (hd::C8_FLOATS, c8_reduce): N = 129 .. 131 only.  Up to 144
    // columns were accepted here once, and columns 131 .. N - 1 were never stored (tests/test_paper_width_shapes_gpu.py, size_s 143).
    if (K != 512 || N <= 128 || N > 131) return hipErrorInvalidValue;
    if (rows) {
        // A = the first row of window 0, lda = the row stride, M = windows: both tile kinds, each storing its own rows
        if (rows_T < 1 || rows_T % 40 || lda * 4 > 0x7fffffffLL || ((long long)M * rows_T - 1) * lda + K > 0x1fffffffLL ||
            (long long)M * ldy * 4 > 0x7fffffffLL)
            return hipErrorInvalidValue;
        const unsigned a_bytes = (unsigned)((((long long)M * rows_T - 1) * lda + K) * 4);
        if (hipError_t e = dynamic_lds<head_rows_kernel<1>, head_rows_kernel<2>>(hd::LDS_BYTES)) return e;
        const HdGather g1{rows, rows_T, M, 0, (unsigned)(lda * 4)}, g2{rows, rows_T, M, 1, (unsigned)(lda * 4)};
        const int ng1 = (M + 15) / 16, ng2 = (M + 3) / 4;
        hipLaunchKernelGGL(head_rows_kernel<1>, dim3(std::min(ng1, num_cus)), dim3(hd::THREADS), hd::LDS_BYTES, s, A, a_bytes, wfrag,
                           bias, Y, ldy, M, N, ng1, g1);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(head_rows_kernel<2>, dim3(std::min(ng2, num_cus)), dim3(hd::THREADS), hd::LDS_BYTES, s, A, a_bytes, wfrag,
                           bias, Y, ldy, M, N, ng2, g2);
        return hipGetLastError();
    }
    if (lda * 4 > 0x7fffffffLL || ((long long)(M - 1) * lda + K) * 4 > 0xffffffffLL || (long long)M * ldy * 4 > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const unsigned a_bytes = (unsigned)(((long long)(M - 1) * lda + K) * 4);
    if (measure_switches().head_trace && !last_only && M % 40 == 0) {
        if (hipError_t e = dynamic_lds<head_ksplit_kernel<0, true>>(hd::LDS_BYTES)) return e;
        hipLaunchKernelGGL((head_ksplit_kernel<0, true>), dim3(std::min(M / 40, num_cus)), dim3(hd::THREADS), hd::LDS_BYTES, s, A,
                           (unsigned)(lda * 4), a_bytes, wfrag, bias, Y, ldy, M, N, M / 40);
        return hipGetLastError();
    }
    if (!last_only) {
        if (M % 40) return hipErrorInvalidValue;
        const int ngroups = M / 40;
        if (hipError_t e = dynamic_lds<head_ksplit_kernel<0>>(hd::LDS_BYTES)) return e;
        hipLaunchKernelGGL(head_ksplit_kernel<0>, dim3(std::min(ngroups, num_cus)), dim3(hd::THREADS), hd::LDS_BYTES, s, A,
                           (unsigned)(lda * 4), a_bytes, wfrag, bias, Y, ldy, M, N, ngroups);
    } else {
        const int ngroups = (M + 3) / 4;
        if (hipError_t e = dynamic_lds<head_ksplit_kernel<2>>(hd::LDS_BYTES)) return e;
        hipLaunchKernelGGL(head_ksplit_kernel<2>, dim3(std::min(ngroups, num_cus)), dim3(hd::THREADS), hd::LDS_BYTES, s, A,
                           (unsigned)(lda * 4), a_bytes, wfrag, bias, Y, ldy, M, N, ngroups);
    }
    return hipGetLastError();
}

}  // namespace tip
