// tip_schedule.hip — which plan(s) a forward takes: AUTO's cost model, the split of a batch into whole rounds + a remainder, the
// recurrence variant.  Pure host arithmetic on (Dims, B, T, #CUs, options): no HIP call, no handle mutation, no allocation.
// tip_abi.hip (forward_impl) runs what schedule_forward answers; tip_debug_schedule shows it without a device.
#include <string.h>

#include "tip_internal.h"

namespace tip {

// The parsing rules of tip_measure.h: e = the variable's value, null when it is unset (always, in the default build).
static bool sw_bool(const char* e, bool def) { return e ? e[0] != '0' : def; }
static int sw_int(const char* e, int def) { return e ? atoi(e) : def; }
static bool sw_not_old(const char* e, bool def) { return e ? strcmp(e, "old") != 0 : def; }

const MeasureSwitches& measure_switches() {
    static const MeasureSwitches sw = [] {
        MeasureSwitches m;
#define TIP_SWITCH(env, type, field, parse, def, doc) m.field = parse(tip_env(env), def);
#include "tip_measure.h"
#undef TIP_SWITCH
        return m;
    }();
    return sw;
}

namespace {

// The cost model's constants: microseconds on one MI355X (256 CUs) at T = 40 — the only window length the window-split plans and the
// rounds + remainder split serve.  They scale with the CU count only through `cus`; of the two encoder rounds only the RATIO matters.
// tools/auto_calibrate.py --stages re-measures every one of them next to the box it runs on.
namespace cost {
// profiles/r04/plan_bench_split.txt (B = 256 step 0.625 ms):
constexpr long long kHybridRound = 527;       // one-window hybrid encoder, one round of #CUs windows
constexpr long long kTwoWindowRound = 1049;   // two-window encoder, one round of 2 x #CUs windows
constexpr long long kTailRound = 96;          // recurrence + output projection per round of #CUs windows
constexpr long long kRoundStep = 615;         // ONE round (B = #CUs) as one launch (tip_round.hip; profiles/round/ab.txt: 0.613-0.616 ms against
                                              // 0.621-0.623 for the three launches), against kHybridRound + kTailRound
static_assert(kRoundStep <= kHybridRound + kTailRound, "the one-launch round is never taken where it is slower than the three launches");
// profiles/r05/f1s_parts.txt (whole forward / its encoder stage; the staircase as a whole: profiles/pool/auto_sweep.txt):
constexpr long long kSplitQuad = 305, kSplitQuadEncoder = 232;   // window-split plan, one window on four CUs (up to #CUs / 4 windows)
constexpr long long kSplitPair = 452, kSplitPairEncoder = 375;   // ... on two CUs (up to #CUs / 2)
constexpr long long kSharedTailExtra = 35;    // what up to 128 more windows add to the whole rounds' recurrence + projection (round 5:
                                              // B = 300 931 -> 911 us with the shared tail)
// The few-stream latency plan's whole forward behind a batch of whole rounds (tools/auto_calibrate.py --stages; round 6, the plan as one
// launch: 147 / 149 / 181 / 241 us for <= 1 / 8 / 16 / 24 windows — a step per window that shares an XCD — then the launch chain's 286
// at 32 and 372 at 44)
long long latency_us(int n) {
    return n <= 8 ? 147LL + n / 4 : n <= 16 ? 181LL : n <= 24 ? 241LL : n <= 32 ? 200LL + (long long)(3.6 * (n - 8)) : 286LL + 10LL * (n - 32);
}
}  // namespace cost

// Few windows: the latency plan up to 32 windows (0.17-0.28 ms), then ONE window on FOUR CUs up to #CUs / 4 windows (0.30 ms per step;
// the latency plan takes 0.36 ms for 40 windows) and on TWO up to #CUs / 2 (0.45 ms against 0.60 for one window per CU) — the
// window-split encoder, T = 40 only; the latency plan again where that does not apply (<= 64 shorter windows, or up to 48 when the
// window-split plan is held to two CUs per window).  plan: TIP_PLAN_LATENCY, TIP_PLAN_FUSED1S, or TIP_PLAN_AUTO = neither.
struct FewWindows {
    int plan;
    bool quad;   // the window-split encoder would put these windows on four CUs each
};
FewWindows few_windows_plan(const Dims& d, int n, int T, int cus, int f1s_parts) {
    const bool quad = fused2_supported(d, T) && f1s_parts != 2 && fused1s_quad_fits(n, cus);
    if (n <= (quad ? 32 : 48) && latency_supported(d, n, T)) return {TIP_PLAN_LATENCY, quad};
    if (fused2_supported(d, T) && fused1s_fits(n, cus)) return {TIP_PLAN_FUSED1S, quad};
    if (latency_supported(d, n, T)) return {TIP_PLAN_LATENCY, quad};   // <= 64 streams: spread each window over many CUs
    return {TIP_PLAN_AUTO, quad};
}

// Whole rounds: one window per workgroup with the hybrid row tiling (no hand-offs), or two windows per workgroup (80 rows = 5 full
// MFMA row blocks) — whichever needs less time for n windows (#CUs is the stream's effective count).
struct Rounds {
    int plan;       // TIP_PLAN_FUSED2 or TIP_PLAN_FUSEDH
    long long us;   // the encoder's rounds
};
Rounds rounds_encoder(const Dims& d, int n, int T, int cus) {
    const long long c = cus, rounds_h = (n + c - 1) / c, rounds_2 = ((n + 1) / 2 + c - 1) / c;
    if (fused2_supported(d, T) && rounds_2 * cost::kTwoWindowRound < rounds_h * cost::kHybridRound) return {TIP_PLAN_FUSED2, rounds_2 * cost::kTwoWindowRound};
    return {TIP_PLAN_FUSEDH, rounds_h * cost::kHybridRound};
}
// n windows as ONE launch sequence of whole rounds: the encoder + recurrence / projection rounds
long long rounds_us(const Dims& d, int n, int T, int cus) { return rounds_encoder(d, n, T, cus).us + cost::kTailRound * ((n + (long long)cus - 1) / cus); }

// The plan n windows take as a launch sequence of their own (never AUTO; plain FUSED only where the caller pinned it), and whether it
// serves them.  (A demoted handle — TIP_OPT_DEMOTED, after a lost hand-off — takes no cooperating kernel: the latency plan's GEMV
// recurrence is one, the window-split encoder another.)
int resolve_plan(const ScheduleIn& in, int n, int* plan_out) {
    const Dims& d = in.d;
    int plan = in.reuse_full ? TIP_PLAN_FUSED2 : in.plan;   // tip_forward_reuse, full windows: the two-window encoder's ring-reading form
    if (plan == TIP_PLAN_AUTO) {
        plan = in.demoted ? TIP_PLAN_AUTO : few_windows_plan(d, n, in.T, in.cus, in.f1s_parts).plan;
        if (plan == TIP_PLAN_AUTO) plan = !fused_supported(d, in.T) ? TIP_PLAN_GENERAL : rounds_encoder(d, n, in.T, in.cus).plan;
    }
    *plan_out = plan;
    if ((plan == TIP_PLAN_FUSED || plan == TIP_PLAN_FUSEDH) && !fused_supported(d, in.T)) return TIP_ERR_UNSUPPORTED_CONFIG;
    if (plan == TIP_PLAN_FUSED2 && !fused2_supported(d, in.T)) return TIP_ERR_UNSUPPORTED_CONFIG;
    if (plan == TIP_PLAN_FUSED1S &&
        !(fused2_supported(d, in.T) && fused1s_fits(n, in.cus) && (in.f1s_parts != 4 || fused1s_quad_fits(n, in.cus))))
        return TIP_ERR_UNSUPPORTED_CONFIG;
    if (plan == TIP_PLAN_LATENCY && !latency_supported(d, n, in.T)) return TIP_ERR_UNSUPPORTED_CONFIG;
    return TIP_OK;
}

int resolve_rnn_cluster(const ScheduleIn& in, int n) {
    if (in.rnn_cluster) return in.rnn_cluster;
    if (in.demoted) return 1;   // one workgroup per 16-window tile: no inter-workgroup hand-off
    // auto: spread one 16-window tile over as many CUs as the tile count leaves idle
    const int ntiles = (n + kRnnTile - 1) / kRnnTile;
    int c = 16;
    while (c > 1 && ntiles * c > in.cus) c >>= 1;
    // rnn_hidden 512: four-row tiles on 4-workgroup clusters at every batch size (76 us at B = 256 against 114 for the best
    // 16-row variant; tools/rnn_variants2.py).  TIP_RNN_ROWS4=0 keeps the 16-row kernels (measurement).
    return measure_switches().rows4 && in.d.R == 512 ? kRnnRows4 : c;
}

}  // namespace

Schedule schedule_forward(const ScheduleIn& in) {
    const Dims& d = in.d;
    const int B = in.B, T = in.T, cus = in.cus;
    const MeasureSwitches& sw = measure_switches();
    Schedule sc{};
    auto part = [&](int i, int first, int count, int rnn_cluster) {
        sc.part[i] = SchedPart{first, count, TIP_PLAN_AUTO, rnn_cluster};
        const int st = resolve_plan(in, count, &sc.part[i].plan);
        if (sc.status == TIP_OK) sc.status = st;
    };
    // AUTO, a batch that is whole rounds of #CUs windows plus a SMALL remainder: the one-window kernel takes a full round (0.53 ms + the
    // tail) for the remainder alone, the few-windows plans a fraction of it.  Whole rounds and remainder then run as two launch
    // sequences (stream-ordered: they share the workspace) when the model says so; every window's result is bit-identical to what its
    // part's plan gives on its own (tests/test_benchmarked_shapes_gpu.py).  TIP_AUTO_SPLIT=0 disables (measurement).  The model is
    // calibrated at T = 40 on the whole device: other window lengths and masked streams take whole rounds.
    if (!in.reuse_full && in.plan == TIP_PLAN_AUTO && !in.demoted && cus == in.num_cus && B > cus && T == 40 && fused_supported(d, T) && fused_has_rnn_ih(d)) {
        const int r = B % cus, bm = B - r;
        const FewWindows rem = few_windows_plan(d, r, T, cus, in.f1s_parts);
        const long long rem_us = rem.plan == TIP_PLAN_LATENCY ? cost::latency_us(r)
                                 : rem.plan == TIP_PLAN_FUSED1S ? (rem.quad ? cost::kSplitQuad : cost::kSplitPair) : -1;
        if (sw.split && rem_us >= 0) {
            // Round 5: a remainder on the window-split encoder shares ONE recurrence and ONE output projection with the whole rounds —
            // the two encoders write their windows' input terms (and arm their HALL rows) side by side in the whole batch's workspace —
            // instead of bringing a 62-us recurrence + a projection launch of its own.  rnn_hidden 512 only (the four-window recurrence,
            // whose per-window results do not depend on the tiling); bit-identical to the two sequences.
            // (the recurrence advances 1, 2 or 4 tiles per cluster together: a third tile costs a fourth's time, and a fifth a second
            // pass — B = 556 measured 1 533 us shared against 1 509: share only where the remainder does not push the whole rounds'
            // tile count per cluster across such a step, or the rounds have a single tile)
            const int tpg_b = ((B + 3) / 4 + 63) / 64, tpg_m = ((bm + 3) / 4 + 63) / 64;
            const bool tiles_ok = cus == 256 && (tpg_b <= 2 || (tpg_b <= 4 && tpg_m >= 3));
            const long long rem_enc_us = rem.quad ? cost::kSplitQuadEncoder : cost::kSplitPairEncoder;
            if (sw.merge && rem.plan == TIP_PLAN_FUSED1S && tiles_ok && d.with_rnn && d.R == 512 && in.rnn_cluster == 0 &&
                rounds_us(d, bm, T, cus) + rem_enc_us + cost::kSharedTailExtra < rounds_us(d, B, T, cus)) {
                sc.nparts = 2;
                sc.shared_tail = true;
                part(0, 0, bm, kRnnRows4);
                part(1, bm, r, kRnnRows4);
                return sc;
            }
            // (a part never needs more workspace than the whole — carve_workspace is monotone, tests/test_host_cpu.py — but a caller's
            // buffer sized by an older library must fall through to the single launch sequence, not fail)
            if (rounds_us(d, bm, T, cus) + rem_us < rounds_us(d, B, T, cus) && carve_workspace(d, bm, T).total_bytes <= in.workspace_bytes &&
                carve_workspace(d, r, T).total_bytes <= in.workspace_bytes) {
                sc.nparts = 2;
                part(0, 0, bm, resolve_rnn_cluster(in, bm));
                part(1, bm, r, resolve_rnn_cluster(in, r));
                return sc;
            }
        }
    }
    sc.nparts = 1;
    part(0, 0, B, resolve_rnn_cluster(in, B));
    // ONE round on the hybrid encoder as ONE launch (tip_round.hip): the whole batch is at most one window per CU of the whole device,
    // the recurrence is the four-row one, the handle is not demoted (every workgroup of that launch waits for others) and
    // TIP_OPT_NO_ROUND_LAUNCH is clear.  Measured (profiles/round/ab.txt, B = 256, T = 40): cost::kRoundStep.
    sc.round_launch = sc.status == TIP_OK && !in.no_round_launch && !in.demoted && !in.reuse_full && sc.part[0].plan == TIP_PLAN_FUSEDH &&
                      sc.part[0].rnn_cluster == kRnnRows4 && cus == in.num_cus && round_launch_shape(d, B, T, cus);
    return sc;
}

}  // namespace tip

extern "C" int tip_debug_schedule(const tip_handle* h, int B, int T, int cus, int reuse_full, size_t workspace_bytes, int* out, int cap) {
    if (!h || B < 1 || T < 1 || !out || cap < 9) return TIP_ERR_INVALID_ARG;
    const tip::Schedule sc = tip::schedule_forward(tip::ScheduleIn{h->d, B, T, cus > 0 ? cus : h->num_cus, h->num_cus, h->plan, h->rnn_cluster,
                                                                   h->f1s_parts, h->demoted != 0, reuse_full != 0, workspace_bytes,
                                                                   h->no_round_launch != 0});
    int* o = out;
    *o++ = sc.nparts;
    *o++ = sc.shared_tail ? 1 : 0;
    *o++ = sc.part[0].rnn_cluster;   // (the parts' values differ only in the measurement build, under TIP_RNN_ROWS4=0)
    for (const tip::SchedPart& p : sc.part) {
        *o++ = p.first; *o++ = p.count; *o++ = p.plan;
    }
    if (cap >= 10) *o++ = sc.round_launch ? 1 : 0;
    return sc.status;
}
