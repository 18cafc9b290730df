// tip_round.hip — ONE launch for a whole forward of one round: the batch is at most one window per CU on the hybrid encoder
// (TIP_PLAN_FUSEDH), rnn_hidden 512, state width 129..131, T <= 40, inference.
//
// The three-launch sequence (fused_encoder_h_kernel, rnn_rows4_kernel<1, ., ., 8>, head_ksplit_kernel) pays two kernel boundaries —
// every CU drains, then waits for the slowest workgroup of the device — and the recurrence's prologue (XCC exchange, 256 KB of W_hh
// into registers) starts only behind the first of them.  Here a workgroup runs three PHASES, with the three kernels' own statements
// (tip_fused_h.h, tip_rnn_rows4_body.inc, tip_head.h: shared, not copied):
//   1. encoder of window blockIdx.x.  Its IH rows and the sentinel words that arm its HALL rows go out write-through (sc1: other XCDs
//      read them inside this launch); every storing wave drains its stores, workgroup barrier, then ONE launch-tagged flag word per
//      window (flags[kRoundFlag0 + window], agent-scope store; the tag is next_rnn_launch_tag()'s, as for the XCC-exchange words).
//   2. recurrence: the workgroup is member `cid` of cluster `group` exactly as rnn_rows4_kernel maps them (members 8 ids apart: one XCD,
//      verified by the XCC exchange).  W_hh is loaded and the exchange runs first; then thread 0 waits — bounded, the usual give-up
//      path — for the flags of the tile's four windows (windows 4 group .. 4 group + 3: encoded by four other workgroups, on other
//      XCDs), joins the workgroup barrier, and every load of the input terms is an agent-coherent one.
//   3. projection of window 4 group + cid (full output: head_ksplit_kernel's MODE 0 group = that window) or, for the last-row output,
//      of the cluster's tile by member 0 (MODE 2 group = the tile's four last rows).  Every wave first waits, bounded, until row T - 1
//      of what it projects holds no sentinel word; all A loads are sc1 (the rows were stored by other workgroups of this launch).
//      Same fragments, same order of sums: the bits of the three launches.  Window lengths the register-resident projection does not
//      serve (T != 40) keep head_gemm_kernel as a launch of its own behind this one.
// A window's flag is cleared by the member that owns the window, after it has seen row T - 1 of the window complete: every member of
// the cluster has then stored its last step, i.e. passed its flag wait.  A REPLAY of the launch from a HIP graph carries the same tag
// and must find no flag of the previous replay.
// All workgroups of the (padded) grid wait on each other, encoder phases included: the launcher asks the runtime's occupancy answer
// for the whole grid and reports hipErrorCooperativeLaunchTooLarge otherwise (the caller then launches the three kernels).
#include "tip_fused_h.h"
#include "tip_head.h"
#include "tip_rnn_rows4.h"

namespace tip {

__device__ unsigned g_spin_timeouts_round;   // see tip_spin_timeouts()
__device__ __forceinline__ void note_spin_timeout(unsigned* err) {
    atomicAdd(&g_spin_timeouts_round, 1u);
    guard_report(err);
}
hipError_t read_spin_timeouts_round(unsigned* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_spin_timeouts_round), sizeof(unsigned));
}

// measurement only (TIP_FUSEDH_TRACE=1, measurement build): [workgroup][entry, encoder published, recurrence done, exit] in
// s_memrealtime ticks (100 MHz, device-wide), then [4096 + workgroup] = XCC id; read through tip_debug_read_fh_wg
__device__ unsigned long long g_round_wg[5 * 1024];

namespace {

constexpr int kRoundFlag0 = 512;    // first window-flag word in the recurrence's flag area (its XCC-exchange words end below 512)
constexpr int kRoundMaxB = 256;     // window flags kRoundFlag0 .. + 255 (rnn_flag_words keeps 1024 words beside the per-step ones)
constexpr int kRoundLds = hd::LDS_BYTES > fz::LDS_BYTES ? hd::LDS_BYTES : fz::LDS_BYTES;
static_assert(2 * kQ4Rows * kQ4LD * (int)sizeof(float) <= kRoundLds, "the recurrence's tile buffers fit the other phases' LDS");

__device__ __forceinline__ unsigned round_flag_value(unsigned etag) { return (etag << 1) | 1u; }

// phase 1: one window; write-through stores; the flag behind them
struct RoundEncCtl {
    static constexpr int kAux = 16;
    int B;
    unsigned* wflags;
    unsigned etag;
    __device__ __forceinline__ int first() const { return blockIdx.x; }
    __device__ __forceinline__ int stride() const { return B; }
    __device__ __forceinline__ void published(int win, int tid) const {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its write-through stores ...
        __syncthreads();                                     // ... before the one lane that signals for all of them
        if (tid == 0) __hip_atomic_store(wflags + win, round_flag_value(etag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// phase 2: the tile's input terms are written inside this launch
struct RoundRnnCtl {
    static constexpr bool kRound = true;
    static constexpr int kIhAux = 16;
    int B;
    const unsigned* wflags;
    unsigned etag;
    unsigned* lost;   // LDS word: bit m = member m of this cluster never showed up in the XCC exchange
    __device__ __forceinline__ void member_lost(int m) const { *lost |= 1u << m; }   // (thread 0)
    // (thread 0, behind the XCC exchange) true when the flags of all the tile's windows carry this launch's tag
    __device__ __forceinline__ bool inputs_ready(int group, unsigned spin_limit, const Guard& gd) const {
        bool ok = true;
        for (int m = 0; m < kQ4Rows; ++m) {
            const int w = group * kQ4Rows + m;
            if (w >= B) break;
            bool here = false;
            for (unsigned spins = 0; spins < spin_limit; ++spins) {
                here = __hip_atomic_load(wflags + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == round_flag_value(etag);
                if (here) break;
                __builtin_amdgcn_s_sleep(4);
            }
            if (!here) {
                note_spin_timeout(gd.err);
                ok = false;
            }
        }
        return ok;
    }
};

template <class Ctl>
__device__ __forceinline__ void rnn_rows4_round_body(const float* __restrict__ ih, const float* __restrict__ whh_frag, float* __restrict__ hall,
                                                     unsigned* __restrict__ flags, int B, int T, int ntiles, int hall_bytes,
                                                     const float* __restrict__ gate, Guard gd, unsigned etag, int abl, int ngroups, Ctl ctl) {
    constexpr int NT = 1, WAVES = 8;
    constexpr bool TRACE = false, BWD = false;
#include "tip_rnn_rows4_body.inc"
}

// Every wave for itself: wait until row T - 1 of window w holds no sentinel word (two 16-byte sc1 loads per lane and poll).  False: gave up.
__device__ __forceinline__ bool round_wait_last_row(__amdgpu_buffer_rsrc_t hrs, int w, int T, unsigned spin_limit) {
    const int lane = threadIdx.x & 63;
    const int voff = (int)(((unsigned)w * (unsigned)T + (unsigned)(T - 1)) * 2048u) + lane * 16;
    for (unsigned spins = 0; spins < spin_limit; ++spins) {
        asm volatile("" ::: "memory");   // (loop-invariant addresses: do not poll a register)
        const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(hrs, voff, 0, 16);
        const u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(hrs, voff + 1024, 0, 16);
        const bool pend = a.x == kRnnSentinel || a.y == kRnnSentinel || a.z == kRnnSentinel || a.w == kRnnSentinel ||
                          b.x == kRnnSentinel || b.y == kRnnSentinel || b.z == kRnnSentinel || b.w == kRnnSentinel;
        if (__builtin_amdgcn_ballot_w64(pend) == 0) return true;
        __builtin_amdgcn_s_sleep(1);
    }
    return false;
}

// phase 3: ONE row group of the projection; the wait for its last rows sits behind the weight loads where the group's first tile does
// not hold them (MODE 0: rows 0 .. 15 of a 40-row window), in front of the body otherwise (MODE 2)
struct RoundHdCtl {
    int g, ngroups;
    __amdgpu_buffer_rsrc_t hrs;
    int w0, nw, T;          // windows whose row T - 1 this group reads: w0 .. w0 + nw - 1
    unsigned spin_limit;
    unsigned* err;
    bool wait_inside;
    __device__ __forceinline__ int first() const { return g; }
    __device__ __forceinline__ int stride() const { return ngroups; }
    __device__ __forceinline__ void wait_rows() const {
        bool ok = true;
        for (int i = 0; i < nw; ++i) ok &= round_wait_last_row(hrs, w0 + i, T, spin_limit);
        if (!ok && (threadIdx.x & 63) == 0) note_spin_timeout(err);   // (what never arrived is read as the sentinel: NaN rows)
    }
    __device__ __forceinline__ void after_weights() const {
        if (wait_inside) wait_rows();
    }
};

}  // namespace

struct RoundArgs {
    const float* wts;
    const float* x_imu;
    const float* x_s;
    const float* keep_mask;
    float keep_scale;
    float* ih;
    float* hall;
    unsigned* flags;
    const float* whh_frag;
    const float* out_frag;
    const float* out_bias;
    float* y;
    int B, T, NI, S, L, wbytes, ih_off_b, hall_bytes, ntiles;
    int head;               // 0: the projection is a launch of its own; 1: full output (MODE 0); 2: last rows (MODE 2)
    unsigned etag;
    Guard gd;
};

template <bool TRACE>
__global__ __launch_bounds__(fz::THREADS) void forward_round_kernel(RoundArgs a) {
    constexpr int CLUSTER = kQ4Cluster;
    const int tid = threadIdx.x;
    const int cid = (blockIdx.x >> 3) % CLUSTER, group = (blockIdx.x & 7) + 8 * ((blockIdx.x >> 3) / CLUSTER);   // (rnn_rows4_kernel's)
    if (TRACE && tid == 0 && blockIdx.x < 1024) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_round_wg[4096 + blockIdx.x] = xcc & 0xf;
        g_round_wg[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
    }
    // TIP_OPT_FAULT_INJECT bit 1: this member never arrives — as a workgroup of this launch it encodes no window either
    if ((a.gd.fault & 2) && group == 0 && cid == 1) return;
    unsigned* wflags = a.flags + kRoundFlag0;
    __shared__ unsigned s_lost;
    if (tid == 0) s_lost = 0u;   // (ordered before phase 2 by the barrier in front of it)

    // ---- phase 1 ----
    if ((int)blockIdx.x < a.B)
        fused_encoder_h_body<false, false, false>(a.wts, a.x_imu, a.x_s, a.keep_mask, a.keep_scale, nullptr, a.ih, reinterpret_cast<unsigned*>(a.hall),
                                                  a.B, a.T, a.NI, a.S, a.L, a.wbytes, a.ih_off_b, FusedTrain{}, RoundEncCtl{a.B, wflags, a.etag});
    if (TRACE && tid == 0 && blockIdx.x < 1024) g_round_wg[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    __syncthreads();   // the encoder's LDS planes become the recurrence's tile buffers

    // ---- phase 2 ---- (clusters past the batch return at once, like the workgroups that pad rnn_rows4_kernel's grid)
    rnn_rows4_round_body(a.ih, a.whh_frag, a.hall, a.flags, a.B, a.T, a.ntiles, a.hall_bytes, nullptr, a.gd, a.etag, 0, a.ntiles,
                         RoundRnnCtl{a.B, wflags, a.etag, &s_lost});
    if (TRACE && tid == 0 && blockIdx.x < 1024) g_round_wg[4 * blockIdx.x + 2] = __builtin_amdgcn_s_memrealtime();

    // ---- phase 3 ----
    const int w = group * kQ4Rows + cid;   // the window this member owns
    const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(a.hall, 0, a.hall_bytes, 0x00020000);
    const unsigned spin_limit = guard_spin_limit(a.gd.fault, 1u << 20);
    __syncthreads();   // the last step's tile buffer becomes the projection's partial sums
    if (a.head == 1) {
        if (w < a.B)
            head_ksplit_body<0, false, 16>(a.hall, 2048u, (unsigned)a.hall_bytes, a.out_frag, a.out_bias, a.y, a.S, a.B * a.T, a.S, a.B,
                                           RoundHdCtl{w, a.B, hrs, w, 1, a.T, spin_limit, a.gd.err, true});
    } else if (a.head == 2) {
        if (cid == 0 && group < a.ntiles) {
            const int nw = a.B - group * kQ4Rows < kQ4Rows ? a.B - group * kQ4Rows : kQ4Rows;
            const RoundHdCtl hc{group, a.ntiles, hrs, group * kQ4Rows, nw, a.T, spin_limit, a.gd.err, false};
            hc.wait_rows();
            head_ksplit_body<2, false, 16>(a.hall + (size_t)(a.T - 1) * 512, (unsigned)a.T * 2048u,
                                           (unsigned)a.hall_bytes - (unsigned)(a.T - 1) * 2048u, a.out_frag, a.out_bias, a.y, a.S, a.B, a.S,
                                           a.ntiles, hc);
        }
    }
    // A member that never arrived projects nothing: the window it owns would keep whatever the output buffer held.  Its partners, who
    // saw it missing, store NaN there instead — never a finite row that is not this call's.
    if (a.head != 0 && group < a.ntiles && s_lost != 0u) {
        for (int m = 0; m < kQ4Rows; ++m) {
            const int wl = group * kQ4Rows + m;
            if (!((s_lost >> m) & 1u) || wl >= a.B) continue;
            const int n = a.head == 1 ? a.T * a.S : a.S;
            float* yl = a.y + (size_t)wl * n;
            for (int i = tid; i < n; i += fz::THREADS) yl[i] = __uint_as_float(kPoisonBits);
        }
    }
    // the owner of a window clears its flag once row T - 1 of the window is complete (see the top of the file)
    if (w < a.B && tid < 64) {
        const bool done = a.head == 1 ? true : round_wait_last_row(hrs, w, a.T, spin_limit);
        if (a.head == 1 || done) {
            if (tid == 0) __hip_atomic_store(wflags + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (tid == 0) {
            note_spin_timeout(a.gd.err);
        }
    }
    if (TRACE && tid == 0 && blockIdx.x < 1024) g_round_wg[4 * blockIdx.x + 3] = __builtin_amdgcn_s_memrealtime();
}
#undef FH_STAMP

bool round_launch_shape(const Dims& d, int B, int T, int num_cus) {
    const int grid = (((B + kQ4Rows - 1) / kQ4Rows + 7) / 8) * 8 * kQ4Cluster;   // whole rounds of 8 clusters (launch_rnn_rows4_nt)
    return fused_supported(d, T) && fused_has_rnn_ih(d) && d.R == 512 && d.S >= 129 && d.S <= 131 && B >= 1 && B <= kRoundMaxB &&
           grid <= num_cus && (long long)(B + 7) * T * 512 * 4 <= 0x7fffffffLL;
}

hipError_t launch_forward_round(const Dims& d, const float* fused_w, const float* x_imu, const float* x_s, const float* keep_mask,
                                float keep_scale, float* ih, float* hall, unsigned* flags, const float* whh_frag, const float* out_frag,
                                const float* out_bias, float* y, int B, int T, int head, int num_cus, const Guard& gd, hipStream_t s) {
    if (!round_launch_shape(d, B, T, num_cus) || (head != 0 && T != 40) || head < 0 || head > 2) return hipErrorInvalidValue;
    if (hipError_t e = dynamic_lds<forward_round_kernel<false>, forward_round_kernel<true>>(kRoundLds)) return e;
    const int ntiles = (B + kQ4Rows - 1) / kQ4Rows;
    const int grid = (ntiles + 7) / 8 * 8 * kQ4Cluster;
    // every workgroup of the grid — encoder phases included — waits for others: all of them must be resident at once
    static PerDeviceInt occ_dev; int& occ = occ_dev.cur();
    if (hipError_t ce = check_coresident(forward_round_kernel<false>, fz::THREADS, (size_t)kRoundLds, grid, num_cus, &occ)) return ce;
    RoundArgs a{fused_w, x_imu, x_s, keep_mask, keep_scale, ih, hall, flags, whh_frag, out_frag, out_bias, y, B, T, d.n_imu_total, d.S, d.L,
                (int)(fused_packed_floats(d) * 4), (int)((fz::LAYER0 + (size_t)d.L * fz::LAYER_FLOATS) * 4), (int)((long long)B * T * 512 * 4),
                ntiles, head, next_rnn_launch_tag(), gd};
    if (measure_switches().fusedh_trace)
        hipLaunchKernelGGL(forward_round_kernel<true>, dim3(grid), dim3(fz::THREADS), kRoundLds, s, a);
    else
        hipLaunchKernelGGL(forward_round_kernel<false>, dim3(grid), dim3(fz::THREADS), kRoundLds, s, a);
    return hipGetLastError();
}

// (read through tip_debug_read_fh_wg, tip_fused.hip)
hipError_t read_round_wg(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_round_wg), sizeof(unsigned long long) * n);
}

}  // namespace tip

