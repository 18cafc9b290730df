// tip_record.hip — session recorder (include/tip_hip.h, "session recorder"): the rows a live pool's wearers were served — the calibrated
// IMU row, the pose the model answered with, whatever else lies in a static [n, w] buffer — logged in HBM one launch behind the frame and
// handed to the host a page at a time.  A consumer BESIDE the frame, as the trackers are: it reads the engine's static buffers and
// changes none of them.  The state is one buffer (the header has the byte layout):
//
//   header | slot heads [n] | page records [P] | free ring [P] | full queue [P] | pages [P][page_rows][W]
//
//   record_reset_kernel     header, heads, records and rings of a buffer of the stated shape; every page free.
//   record_open_kernel      listed slots start a session (one thread per entry).
//   record_close_kernel     listed slots stop; a partly filled page goes onto the full queue (one thread per entry).
//   record_append_kernel<V> the per-frame launch: one wave per slot.  Lane 0 takes a page when the slot has none (ONE atomic add on the
//                           free ring's head, checked against its tail, taken back when nothing was free), the wave copies row `slot`
//                           of every source behind one another, lane 0 counts the row and, when the page is full, pushes it onto the
//                           full queue (one atomic add on its tail).  With no page free the row is counted as dropped and written nowhere.
//   record_drain_kernel     the pages now on the full queue into a staging buffer, back onto the free ring, the queue advanced.
//
// Nothing here waits: no kernel polls a word another workgroup writes.  Within one append the only words two workgroups touch are the two
// ring counters, by atomics; everything else a workgroup reads was written by an earlier launch.  The drain's workgroups all read the
// counters as the previous launch left them; the LAST one to finish — told so by the value an atomic increment returns, not by looking
// again — moves them.  So a drain must not overlap an append, an open or a close: they are ordered by the stream they share.
// When FEWER pages are free than slots ask in one frame, exactly min(free, asking) slots get one — a claim succeeds only below the tail,
// successful claims take distinct ring entries, and a claim is taken back only after it failed, so the head never reads lower than the
// claims that succeeded — and the others count their row; only WHICH slots get one is not defined.
#include "tip_internal.h"

namespace tip {
namespace rec {

constexpr int kMagic = 0x52454331;          // "REC1"
constexpr int kHdrWords = 16;               // 64 bytes
constexpr int kHeadWords = 8;               // 32 bytes per slot
constexpr int kRecWords = 8;                // 32 bytes per page
constexpr int kMaxSrcs = TIP_RECORD_MAX_SOURCES;
constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / 64;
constexpr int kDrainMaxY = 16;              // chunks of one page copied side by side

// header words
enum { H_MAGIC, H_N, H_PAGES, H_ROWS, H_WIDTH, H_FREE_HEAD, H_FREE_TAIL, H_FULL_HEAD, H_FULL_TAIL, H_DRAIN_DONE };
// slot head words
enum { S_OPEN, S_SESSION, S_ROWS, S_PAGE, S_FILL, S_DROPPED, S_GAPS, S_GAP };
// page record words
enum { R_SLOT, R_SESSION, R_SEQ, R_ROWS, R_GAP };

struct Layout {
    size_t heads, recs, free_ring, full_q, pages, total;   // byte offsets
};

__host__ __device__ inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

__host__ __device__ inline Layout layout(int n, int pages, int page_rows, int width) {
    Layout l;
    l.heads = kHdrWords * 4;
    l.recs = l.heads + (size_t)n * kHeadWords * 4;
    l.free_ring = l.recs + (size_t)pages * kRecWords * 4;
    l.full_q = l.free_ring + up16((size_t)pages * 4);
    l.pages = l.full_q + up16((size_t)pages * 4);
    l.total = l.pages + (size_t)pages * page_rows * width * 4;
    return l;
}

struct Sources {
    tip_record_source s[kMaxSrcs];
    int count;
};

// the buffer is one this file laid out for n slots: every offset below then stays inside tip_record_state_bytes(n, P, R, W)
__device__ __forceinline__ bool header_ok(const int* hdr, int n) {
    return hdr[H_MAGIC] == kMagic && hdr[H_N] == n && hdr[H_PAGES] >= 1 && hdr[H_ROWS] >= 1 && hdr[H_WIDTH] >= 1;
}

__global__ __launch_bounds__(kThreads) void record_reset_kernel(int* __restrict__ st, int n, int pages, int page_rows, int width) {
    const Layout l = layout(n, pages, page_rows, width);
    int* heads = st + l.heads / 4;
    int* recs = st + l.recs / 4;
    int* ring = st + l.free_ring / 4;
    int* fq = st + l.full_q / 4;
    const size_t step = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < (size_t)n * kHeadWords; i += step)
        heads[i] = (i % kHeadWords) == S_PAGE ? -1 : 0;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < (size_t)pages * kRecWords; i += step)
        recs[i] = (i % kRecWords) == R_SLOT ? -1 : 0;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < (size_t)pages; i += step) {
        ring[i] = (int)i;
        fq[i] = -1;
    }
    if (blockIdx.x == 0 && threadIdx.x < kHdrWords) {
        const int t = threadIdx.x;
        st[t] = t == H_MAGIC ? kMagic : t == H_N ? n : t == H_PAGES ? pages : t == H_ROWS ? page_rows : t == H_WIDTH ? width
                : t == H_FREE_TAIL ? pages : 0;
    }
}

__global__ __launch_bounds__(kThreads) void record_open_kernel(int* __restrict__ st, int n, const int* __restrict__ slots,
                                                                const int* __restrict__ sessions, int count) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= count || !header_ok(st, n)) return;
    const int slot = slots[j];
    if (slot < 0 || slot >= n) return;
    int* h = st + kHdrWords + (size_t)slot * kHeadWords;
    if (h[S_OPEN]) return;                      // (the host refuses it first; an open session is never replaced)
    h[S_OPEN] = 1;
    h[S_SESSION] = sessions[j];
    h[S_ROWS] = 0;
    h[S_PAGE] = -1;
    h[S_FILL] = 0;
    h[S_DROPPED] = 0;
    h[S_GAPS] = 0;
    h[S_GAP] = 0;
}

// a page onto the full queue: at most P pages exist and each is on the free ring, with a slot or on the queue, so the queue never laps
__device__ __forceinline__ void push_full(int* st, const Layout& l, int pages, int page) {
    const unsigned t = atomicAdd(reinterpret_cast<unsigned*>(st + H_FULL_TAIL), 1u);
    (st + l.full_q / 4)[t % (unsigned)pages] = page;
}

__global__ __launch_bounds__(kThreads) void record_close_kernel(int* __restrict__ st, int n, const int* __restrict__ slots, int count) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= count || !header_ok(st, n)) return;
    const int slot = slots[j];
    if (slot < 0 || slot >= n) return;
    int* h = st + kHdrWords + (size_t)slot * kHeadWords;
    if (!h[S_OPEN]) return;
    const int pages = st[H_PAGES];
    const Layout l = layout(n, pages, st[H_ROWS], st[H_WIDTH]);
    const int page = h[S_PAGE];
    if (page >= 0 && page < pages) push_full(st, l, pages, page);      // (its record already holds the rows used)
    h[S_PAGE] = -1;
    h[S_FILL] = 0;
    h[S_OPEN] = 0;
}

// V = float4: every source's columns and stride are multiples of 4 floats and every base is 16-byte aligned (the host's choice, per launch)
template <class V>
__global__ __launch_bounds__(kThreads) void record_append_kernel(int* __restrict__ st, int n, Sources src, const int* __restrict__ valid,
                                                                  int valid_min) {
    constexpr int per = sizeof(V) / 4;
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);          // (uniform over the wave)
    if (slot >= n || !header_ok(st, n)) return;
    const int pages = st[H_PAGES], page_rows = st[H_ROWS], width = st[H_WIDTH];
    int w_src = 0;
    for (int s = 0; s < src.count; ++s) w_src += src.s[s].cols;
    if (w_src != width) return;                 // the table is not the one this buffer was laid out for: nothing is written
    int* h = st + kHdrWords + (size_t)slot * kHeadWords;
    if (!h[S_OPEN]) return;
    if (valid && valid[slot] < valid_min) return;
    const Layout l = layout(n, pages, page_rows, width);
    int* recs = st + l.recs / 4;
    int page = h[S_PAGE], fill = h[S_FILL];
    const int rows = h[S_ROWS];
    if (page < 0) {
        // lane 0 asks the free ring; the answer (a page, or -1) goes to the wave
        int got = -1;
        if (lane == 0) {
            unsigned* head = reinterpret_cast<unsigned*>(st + H_FREE_HEAD);
            const unsigned tail = (unsigned)st[H_FREE_TAIL];                     // (only a drain moves it, and none runs beside us)
            const unsigned old = atomicAdd(head, 1u);
            if ((int)(tail - old) > 0) {
                got = (st + l.free_ring / 4)[old % (unsigned)pages];
            } else {
                atomicSub(head, 1u);                                            // nothing was free: the claim is taken back
            }
            if (got >= 0 && got < pages) {
                int* r = recs + (size_t)got * kRecWords;
                r[R_SLOT] = slot;
                r[R_SESSION] = h[S_SESSION];
                r[R_SEQ] = rows / page_rows;                                    // (every earlier page of the session was full)
                r[R_ROWS] = 0;
                r[R_GAP] = h[S_GAP];                                            // rows dropped in front of this page's first row
                h[S_GAP] = 0;
                h[S_PAGE] = got;
            } else {
                got = -1;
                if (h[S_GAP] == 0) h[S_GAPS] += 1;
                h[S_GAP] += 1;
                h[S_DROPPED] += 1;
            }
        }
        page = __shfl(got, 0);
        fill = 0;
        if (page < 0) return;
    }
    if (page >= pages || fill < 0 || fill >= page_rows) return;                 // (a head this file never writes: nothing is stored)
    V* dst = reinterpret_cast<V*>(reinterpret_cast<unsigned char*>(st) + l.pages) + ((size_t)page * page_rows + fill) * (width / per);
    for (int s = 0; s < src.count; ++s) {
        const int cv = src.s[s].cols / per;
        const V* from = reinterpret_cast<const V*>(src.s[s].data + (size_t)slot * src.s[s].stride);
        for (int c = lane; c < cv; c += 64) dst[c] = from[c];
        dst += cv;
    }
    if (lane == 0) {
        fill += 1;
        (recs + (size_t)page * kRecWords)[R_ROWS] = fill;
        h[S_ROWS] = rows + 1;
        if (fill == page_rows) {
            push_full(st, l, pages, page);
            h[S_PAGE] = -1;
            fill = 0;
        }
        h[S_FILL] = fill;
    }
}

// one page (or a record) as vectors of V, strided over the workgroups of gridDim.y
template <class V>
__device__ __forceinline__ void drain_copy(const float* __restrict__ from, float* __restrict__ to, size_t floats) {
    const size_t vecs = floats / (sizeof(V) / 4);
    const V* f = reinterpret_cast<const V*>(from);
    V* t = reinterpret_cast<V*>(to);
    for (size_t i = (size_t)blockIdx.y * kThreads + threadIdx.x; i < vecs; i += (size_t)gridDim.y * kThreads) t[i] = f[i];
}

// staging: 16 header words | max_pages records | max_pages pages.  One workgroup column per queue entry, its page's chunks over gridDim.y;
// 16-byte vectors when a page is a multiple of 16 bytes (then every page of the pool and of the staging buffer starts on one).
__global__ __launch_bounds__(kThreads) void record_drain_kernel(int* __restrict__ st, int* __restrict__ staging, int max_pages,
                                                                 int* __restrict__ out_count) {
    const int n = st[H_N], pages = st[H_PAGES], page_rows = st[H_ROWS], width = st[H_WIDTH];
    if (st[H_MAGIC] != kMagic || n < 0 || pages < 1 || page_rows < 1 || width < 1) return;      // (uniform over the grid)
    const Layout l = layout(n, pages, page_rows, width);
    const unsigned head = (unsigned)st[H_FULL_HEAD], tail = (unsigned)st[H_FULL_TAIL];
    const unsigned ftail = (unsigned)st[H_FREE_TAIL];
    const int avail = (int)(tail - head);
    const int count = avail < max_pages ? (avail < 0 ? 0 : avail) : max_pages;
    const int j = blockIdx.x;
    if (j < count) {
        const int page = (st + l.full_q / 4)[(head + (unsigned)j) % (unsigned)pages];
        if (page >= 0 && page < pages) {
            const size_t page_floats = (size_t)page_rows * width;
            const float* from = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(st) + l.pages) + (size_t)page * page_floats;
            float* to = reinterpret_cast<float*>(staging + kHdrWords + (size_t)max_pages * kRecWords) + (size_t)j * page_floats;
            if (page_floats & 3)
                drain_copy<float>(from, to, page_floats);
            else
                drain_copy<float4>(from, to, page_floats);
            if (blockIdx.y == 0) {
                if (threadIdx.x < kRecWords)
                    (staging + kHdrWords + (size_t)j * kRecWords)[threadIdx.x] = (st + l.recs / 4)[(size_t)page * kRecWords + threadIdx.x];
                // back onto the free ring: entries from its tail on are unused until the tail moves (below, by the last workgroup)
                if (threadIdx.x == 0) (st + l.free_ring / 4)[(ftail + (unsigned)j) % (unsigned)pages] = page;
            }
        }
    }
    // the last workgroup to get here moves the counters: every other one has read them by now and reads nothing of the state again
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned total = gridDim.x * gridDim.y;
        const unsigned old = atomicInc(reinterpret_cast<unsigned*>(st + H_DRAIN_DONE), total - 1);      // (wraps to 0 at the last arrival)
        if (old == total - 1) {
            st[H_FULL_HEAD] = (int)(head + (unsigned)count);
            st[H_FREE_TAIL] = (int)(ftail + (unsigned)count);
            staging[0] = count;
            staging[1] = avail - count;                                          // pages still on the queue
            staging[2] = pages - (int)(ftail + (unsigned)count - (unsigned)st[H_FREE_HEAD]);   // pages in use after this drain
            staging[3] = n;
            staging[4] = pages;
            staging[5] = page_rows;
            staging[6] = width;
            staging[7] = max_pages;
            if (out_count) *out_count = count;
        }
    }
}

}  // namespace rec
}  // namespace tip

using namespace tip;
using namespace tip::rec;

static bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static bool bad_shape(int n, int pages, int page_rows, int width) {
    if (n < 0 || tip_bad_count(n) || pages < 1 || tip_bad_count(pages) || page_rows < 1 || page_rows > (1 << 20) || width < 1 ||
        width > (1 << 20))
        return true;
    return (double)pages * page_rows * width * 4.0 > 6.0e10;      // (no page pool beyond 60 GB: every offset stays far inside size_t)
}

extern "C" {

int tip_record_state_bytes(int n_slots, int pages, int page_rows, int width, size_t* bytes) {
    if (!bytes || bad_shape(n_slots, pages, page_rows, width)) return TIP_ERR_INVALID_ARG;
    *bytes = layout(n_slots, pages, page_rows, width).total;
    return TIP_OK;
}

int tip_record_staging_bytes(int max_pages, int page_rows, int width, size_t* bytes) {
    if (!bytes || bad_shape(0, max_pages, page_rows, width)) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)kHdrWords * 4 + (size_t)max_pages * kRecWords * 4 + (size_t)max_pages * page_rows * width * 4;
    return TIP_OK;
}

int tip_record_reset(void* state, int n_slots, int pages, int page_rows, int width, tip_stream_t stream) {
    if (!state || !aligned_to(state, 16) || bad_shape(n_slots, pages, page_rows, width)) return TIP_ERR_INVALID_ARG;
    const size_t most = (size_t)(n_slots > pages ? n_slots : pages) * kHeadWords;
    const unsigned grid = (unsigned)((most + kThreads - 1) / kThreads < 1024 ? (most + kThreads - 1) / kThreads : 1024);
    hipLaunchKernelGGL(record_reset_kernel, dim3(grid < 1 ? 1 : grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<int*>(state), n_slots, pages, page_rows, width);
    return tip_launch_status();
}

int tip_record_open(void* state, int n_slots, const int* slots, const int* sessions, int count, tip_stream_t stream) {
    if (!state || !aligned_to(state, 16) || n_slots < 0 || tip_bad_count(n_slots) || tip_bad_count(count)) return TIP_ERR_INVALID_ARG;
    if (count > 0 && (!slots || !sessions || !aligned_to(slots, 4) || !aligned_to(sessions, 4))) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(record_open_kernel, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<int*>(state), n_slots, slots, sessions, count);
    return tip_launch_status();
}

int tip_record_close(void* state, int n_slots, const int* slots, int count, tip_stream_t stream) {
    if (!state || !aligned_to(state, 16) || n_slots < 0 || tip_bad_count(n_slots) || tip_bad_count(count)) return TIP_ERR_INVALID_ARG;
    if (count > 0 && (!slots || !aligned_to(slots, 4))) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(record_close_kernel, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<int*>(state), n_slots, slots, count);
    return tip_launch_status();
}

int tip_record_append(void* state, int n_slots, const tip_record_source* srcs, int n_srcs, const int* valid, int valid_min,
                      tip_stream_t stream) {
    if (!state || !aligned_to(state, 16) || n_slots < 0 || tip_bad_count(n_slots) || !srcs || n_srcs < 1 || n_srcs > kMaxSrcs ||
        !aligned_to(valid, 4))
        return TIP_ERR_INVALID_ARG;
    Sources tab = {};
    tab.count = n_srcs;
    bool wide = true;
    long long width = 0;
    for (int s = 0; s < n_srcs; ++s) {
        const tip_record_source& e = srcs[s];
        if (!e.data || !aligned_to(e.data, 4) || e.cols < 1 || e.cols > (1 << 20) || e.stride < e.cols) return TIP_ERR_INVALID_ARG;
        wide = wide && !(e.cols & 3) && !(e.stride & 3) && aligned_to(e.data, 16);
        width += e.cols;
        tab.s[s] = e;
    }
    if (width < 1 || width > (1 << 20)) return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    const dim3 grid((n_slots + kWavesPerBlock - 1) / kWavesPerBlock);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (wide)
        hipLaunchKernelGGL(record_append_kernel<float4>, grid, dim3(kThreads), 0, s, static_cast<int*>(state), n_slots, tab, valid, valid_min);
    else
        hipLaunchKernelGGL(record_append_kernel<float>, grid, dim3(kThreads), 0, s, static_cast<int*>(state), n_slots, tab, valid, valid_min);
    return tip_launch_status();
}

int tip_record_drain(void* state, void* staging, int max_pages, int* out_count, tip_stream_t stream) {
    if (!state || !staging || !aligned_to(state, 16) || !aligned_to(staging, 16) || !aligned_to(out_count, 4) || max_pages < 1 ||
        tip_bad_count(max_pages))
        return TIP_ERR_INVALID_ARG;
    hipLaunchKernelGGL(record_drain_kernel, dim3(max_pages, kDrainMaxY), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<int*>(state), static_cast<int*>(staging), max_pages, out_count);
    return tip_launch_status();
}

}  // extern "C"
