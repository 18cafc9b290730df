// tip_handover.hip — wearer hand-over (include/tip_hip.h, "hand-over"): a live slot's state blocks copied out of the buffers of one pool
// and into those of another, so that a wearer continues where it was — bit for bit — in a pool of another size, on another device (through
// the host) or after a restart.  Every per-wearer state of the library is "n fixed blocks of *_state_bytes(1, ...) bytes in one buffer":
// the stream block (tip_stream.h), the calibration and fill blocks, the packet ring and clock envelope, the tracker carry and the terrain
// block.  None of them stores its own slot index or anything derived from n, so a block moves as bytes; the ONE word that belongs to the
// buffer and not to the wearer is the stream block's shape word (sz::SHP at 40 rows, word 2 at any other length), which
// tip_handover_stream_import leaves in place and compares first: a block recorded under another shape or window never lands.
//
//   handover_copy_kernel<V, STREAM>   export (state block slots[j] -> row j) and import (row j -> state block slots[j]) in one body.
//
// One workgroup per (list entry, chunk of kChunk vectors), the chunks of an entry strided over gridDim.y; the slot index is one scalar load
// per workgroup; V is uint4 (16 B per lane) when block size, both strides and both bases allow it, unsigned (4 B) otherwise — chosen per
// launch by the host.  No LDS, no barrier, nothing waits on another workgroup.  A list entry outside [0, n_slots) is skipped (the
// convention of tip_stream_history_override): its row (export) or block (import) is left as it was.  Reads and writes stay inside
// block slots[j] of `state` and inside bytes [j * stride, j * stride + block_bytes) of the rows.
#include "tip_stream.h"

namespace tip {

constexpr int kHandoverThreads = 256;
constexpr int kHandoverChunk = 4 * kHandoverThreads;   // vectors per chunk: four loads of a lane in flight
constexpr int kHandoverMaxY = 64;                      // chunks of one entry served side by side; the rest by the stride loop

// one vector to dst[i]; STREAM: the vector that holds the shape word (word `shp` of the block) is stored word by word without it
template <class V, bool STREAM>
__device__ __forceinline__ void handover_put(V* __restrict__ dst, size_t i, V v, int shp) {
    constexpr int per = sizeof(V) / 4;                      // 4-byte words per vector
    if (STREAM && i == (size_t)(shp / per)) {
        unsigned w[per];
        __builtin_memcpy(w, &v, sizeof(V));
        unsigned* d4 = reinterpret_cast<unsigned*>(dst + i);
#pragma unroll
        for (int e = 0; e < per; ++e)
            if (e != shp % per) d4[e] = w[e];
        return;
    }
    dst[i] = v;
}

// STREAM (import only): `shp` is the index of the block's shape word in 4-byte words, `win` the window length the caller states.
template <class V, bool STREAM>
__global__ __launch_bounds__(kHandoverThreads) void handover_copy_kernel(unsigned char* __restrict__ state, int n_slots, size_t block_bytes,
                                                                          const int* __restrict__ slots, unsigned char* __restrict__ rows,
                                                                          size_t row_stride, int to_state, int shp, int win,
                                                                          int* __restrict__ refused) {
    const int j = blockIdx.x;
    const int slot = slots[j];                              // (uniform: one scalar load per workgroup)
    if (slot < 0 || slot >= n_slots) {
        if (STREAM && refused && blockIdx.y == 0 && threadIdx.x == 0) refused[j] = -1;
        return;
    }
    unsigned char* blk = state + (size_t)slot * block_bytes;
    unsigned char* row = rows + (size_t)j * row_stride;
    if (STREAM) {
        // the destination's word decides: the incoming block must have been recorded under the same shape and window, and (any-length
        // layout) block 0 must confirm the stride that led to this block, as stream_check does for every other kernel of that layout
        const int mine = reinterpret_cast<const int*>(blk)[shp], theirs = reinterpret_cast<const int*>(row)[shp];
        bool ok = mine == theirs;
        if (win != sz::WIN) {
            const int w0 = reinterpret_cast<const int*>(state)[shp];
            ok = ok && (w0 >> 16) == sz::WTAG && ((w0 >> 2) & 0x3fff) == win && mine == w0;
        } else {
            ok = ok && (mine >> 2) == 0;
        }
        if (refused && blockIdx.y == 0 && threadIdx.x == 0) refused[j] = ok ? -1 : slot;
        if (!ok) return;
    }
    const V* src = reinterpret_cast<const V*>(to_state ? row : blk);
    V* dst = reinterpret_cast<V*>(to_state ? blk : row);
    const size_t nvec = block_bytes / sizeof(V);
    for (size_t c = blockIdx.y; c * kHandoverChunk < nvec; c += gridDim.y) {
        // four loads of a lane go out before its first store (named values: an indexed array here was placed in LDS by the compiler)
        const size_t i0 = c * kHandoverChunk + threadIdx.x, i1 = i0 + kHandoverThreads, i2 = i1 + kHandoverThreads, i3 = i2 + kHandoverThreads;
        V v0 = {}, v1 = {}, v2 = {}, v3 = {};
        if (i0 < nvec) v0 = src[i0];
        if (i1 < nvec) v1 = src[i1];
        if (i2 < nvec) v2 = src[i2];
        if (i3 < nvec) v3 = src[i3];
        if (i0 < nvec) handover_put<V, STREAM>(dst, i0, v0, shp);
        if (i1 < nvec) handover_put<V, STREAM>(dst, i1, v1, shp);
        if (i2 < nvec) handover_put<V, STREAM>(dst, i2, v2, shp);
        if (i3 < nvec) handover_put<V, STREAM>(dst, i3, v3, shp);
    }
}

}  // namespace tip

using namespace tip;

static bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Every refusal of the three entry points, then the launch.  shp < 0: the generic pair.
static int handover_launch(void* state, int n_slots, size_t block_bytes, const int* slots, int count, void* rows, size_t row_stride,
                           int to_state, int shp, int win, int* refused, tip_stream_t stream) {
    if (!state || !rows || n_slots < 0 || tip_bad_count(count) || (count > 0 && !slots)) return TIP_ERR_INVALID_ARG;
    if (block_bytes == 0 || (block_bytes & 3) || row_stride < block_bytes || (row_stride & 3)) return TIP_ERR_INVALID_ARG;
    if (!aligned_to(state, 4) || !aligned_to(rows, 4) || !aligned_to(slots, 4) || !aligned_to(refused, 4)) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    const bool wide = !(block_bytes & 15) && !(row_stride & 15) && aligned_to(state, 16) && aligned_to(rows, 16);
    const size_t nvec = block_bytes / (wide ? 16 : 4), chunks = (nvec + kHandoverChunk - 1) / kHandoverChunk;
    const dim3 grid(count, (unsigned)(chunks < (size_t)kHandoverMaxY ? chunks : (size_t)kHandoverMaxY));
    auto* st = static_cast<unsigned char*>(state);
    auto* rw = static_cast<unsigned char*>(rows);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (shp < 0) {
        if (wide)
            hipLaunchKernelGGL((handover_copy_kernel<uint4, false>), grid, dim3(kHandoverThreads), 0, s, st, n_slots, block_bytes, slots, rw,
                               row_stride, to_state, 0, 0, nullptr);
        else
            hipLaunchKernelGGL((handover_copy_kernel<unsigned, false>), grid, dim3(kHandoverThreads), 0, s, st, n_slots, block_bytes, slots, rw,
                               row_stride, to_state, 0, 0, nullptr);
    } else {
        if (wide)
            hipLaunchKernelGGL((handover_copy_kernel<uint4, true>), grid, dim3(kHandoverThreads), 0, s, st, n_slots, block_bytes, slots, rw,
                               row_stride, 1, shp, win, refused);
        else
            hipLaunchKernelGGL((handover_copy_kernel<unsigned, true>), grid, dim3(kHandoverThreads), 0, s, st, n_slots, block_bytes, slots, rw,
                               row_stride, 1, shp, win, refused);
    }
    return tip_launch_status();
}

extern "C" {

int tip_handover_export(const void* state, int n_slots, size_t block_bytes, const int* slots, int count, void* out, size_t out_stride,
                        tip_stream_t stream) {
    return handover_launch(const_cast<void*>(state), n_slots, block_bytes, slots, count, out, out_stride, 0, -1, 0, nullptr, stream);
}

int tip_handover_import(void* state, int n_slots, size_t block_bytes, const int* slots, int count, const void* in, size_t in_stride,
                        tip_stream_t stream) {
    return handover_launch(state, n_slots, block_bytes, slots, count, const_cast<void*>(in), in_stride, 1, -1, 0, nullptr, stream);
}

int tip_handover_stream_import(void* state, int n_streams, const int* slots, int count, const void* in, size_t in_stride, int window,
                               int* refused, tip_stream_t stream) {
    if (window < 1 || window > sz::WIN_MAX) return TIP_ERR_INVALID_ARG;
    const size_t block_bytes = (size_t)stream_lay(window).stride * sizeof(float);
    return handover_launch(state, n_streams, block_bytes, slots, count, const_cast<void*>(in), in_stride, 1, window == sz::WIN ? sz::SHP : 2,
                           window, refused, stream);
}

}  // extern "C"
