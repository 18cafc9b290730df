// tip_rnn_rows4.h — what the two users of the four-row-tile recurrence share beside its statements: the stand-alone kernel
// (rnn_rows4_kernel, tip_general.hip: the design is described there) and the one-launch round (forward_round_kernel, tip_round.hip).
// The statements are tip_rnn_rows4_body.inc, included by both inside a function with the kernel's parameter names, the template
// parameters NT, TRACE, BWD, WAVES, a type Ctl and an object ctl (below), and note_spin_timeout(unsigned*) of the including file (its
// own give-up counter) in scope.  (Text, not a call: see fused_encoder_h_body, tip_fused_h.h.)
#pragma once
#include "tip_internal.h"
#include "tip_layernorm.h"

namespace tip {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned kRnnSentinel = 0xFFFFFFFFu;   // HALL is pre-filled with it: a NaN bit pattern no arithmetic produces (rnn_resident_kernel)
constexpr int kQ4Rows = 4, kQ4Cluster = 4, kQ4Tiles = 4, kQ4LD = 512 + 16;

// Where a member's input terms come from.  RnnFromMemory is the stand-alone kernel's: an earlier launch wrote them, plain loads,
// requested at entry.  The one-launch round has a control of its own (tip_round.hip): the terms are written by other workgroups of
// the SAME launch, so thread 0 waits (bounded) for the tile's window flags behind the XCC exchange, and every load of them is an
// agent-coherent one (kIhAux = 16, sc1).
struct RnnFromMemory {
    static constexpr bool kRound = false;
    static constexpr int kIhAux = 0;
    __device__ __forceinline__ bool inputs_ready(int, unsigned, const Guard&) const { return true; }
    __device__ __forceinline__ void member_lost(int) const {}
};

// measurement only (TIP_RNN_TRACE=1; defined in tip_general.hip, touched by the TRACE instantiations alone)
extern __device__ unsigned long long g_rnn_trace[2048];

}  // namespace tip
