// tip_abi.hip — the C-ABI of libtip_hip.so (include/tip_hip.h): handle, workspace carve-up and the forward's launch
// sequences (the packed weight image is tip_pack.hip's).  No torch types, no exceptions across the boundary.
#include <math.h>
#include <string.h>

#include <new>

#include <mutex>
#include "tip_internal.h"
#include <atomic>
#include <chrono>

using namespace tip;

namespace {

const char* kStatusText[] = {
    "ok",
    "invalid argument",
    "unsupported configuration",
    "not ready: no packed weights attached",
    "workspace too small or misaligned",
    "HIP runtime error",
    "no HIP device",
    "allocation failure",
    "an inter-workgroup hand-off wait gave up in an earlier launch (outputs of that launch are NaN-poisoned); tip_check(h, 1) clears",
};

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

void build_tensor_table(tip_handle* h) {
    const Dims& d = h->d;
    auto add = [&](const std::string& n, int r, int cdim) {
        h->tensor_names.push_back(n);
        h->tensor_shapes.push_back({r, cdim});
    };
    add("in_linear.weight", d.D, d.In);
    add("in_linear.bias", d.D, 0);
    for (int l = 0; l < d.L; ++l) {
        const std::string p = "tf_encode.layers." + std::to_string(l) + ".";
        add(p + "self_attn.in_proj_weight", 3 * d.D, d.D);
        add(p + "self_attn.in_proj_bias", 3 * d.D, 0);
        add(p + "self_attn.out_proj.weight", d.D, d.D);
        add(p + "self_attn.out_proj.bias", d.D, 0);
        add(p + "linear1.weight", d.F, d.D);
        add(p + "linear1.bias", d.F, 0);
        add(p + "linear2.weight", d.D, d.F);
        add(p + "linear2.bias", d.D, 0);
        add(p + "norm1.weight", d.D, 0);
        add(p + "norm1.bias", d.D, 0);
        add(p + "norm2.weight", d.D, 0);
        add(p + "norm2.bias", d.D, 0);
    }
    if (d.with_rnn) {
        add("rnn.weight_ih_l0", d.R, d.D);
        add("rnn.weight_hh_l0", d.R, d.R);
        add("rnn.bias_ih_l0", d.R, 0);
        add("rnn.bias_hh_l0", d.R, 0);
        add("linear.weight", d.S, d.R);
    } else {
        add("linear.weight", d.S, d.D);
    }
    add("linear.bias", d.S, 0);
}

}  // namespace
Workspace tip::carve_workspace(const Dims& d, int B, int T) {
    Workspace w;
    const size_t M = (size_t)B * T;
    const size_t Mp = align_up(M, 16);
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off = align_up(off + n, 64); return o; };
    int big = 3 * d.D;
    if (d.F > big) big = d.F;
    if (d.R > big) big = d.R;
    if (d.InPad > big) big = d.InPad;
    w.flow = take(fused_supported(d, 40) && fused_has_rnn_ih(d) ? latency_flow_flag_floats() : 0);   // first: offset 0 whatever B and T are
    w.xa = take(Mp * d.D);
    w.xb = take(Mp * d.D);
    w.big = take(Mp * big);
    w.att = take(Mp * d.D);
    w.hall = take(Mp * (d.with_rnn ? d.R : 1));
    w.flags = take(rnn_flag_words(B, T) + 64);
    w.lat = take(latency_supported(d, B, T) ? latency_workspace_floats(B, T) : 0);   // (the persistent variant uses the same buffers)
    // window-split / pair-split plans: partial-sum images the partner workgroups exchange.  Only batches whose workgroups can all be
    // resident use them (2 x ceil(B / 2) <= #CUs <= 256), so the section stops growing at 256 windows — and does not shrink beyond:
    // AUTO runs a batch of whole rounds + a remainder as two forwards over the SAME workspace, and a part must never need more than
    // the whole (until round 4 the section was sized for B <= 1024, 168 MB at B = 1024, and absent above: a 1064-window batch
    // whose 1024-window part asked for more than the whole got TIP_ERR_WORKSPACE).
    w.xchg = take(fused2_supported(d, T) ? fused2s_xchg_floats(B < 256 ? B : 256) : 0);
    w.total_bytes = off * sizeof(float);
    return w;
}
namespace {

int fail_hip(tip_handle* h, hipError_t e, const char* where) {
    h->last_hip_error = std::string(where) + ": " + hipGetErrorString(e);
    return TIP_ERR_HIP;
}

// profile == 1: every stage; profile == 2: only the dominant stage of the active plan (cheap enough to leave on
// inside a timed region).  One event pair per launch, accumulated until tip_set_option(TIP_OPT_PROFILE, ...).
bool stage_is_dominant(const char* name) {
    return !strcmp(name, "fused_encoder") || !strcmp(name, "ffn1_gemm");
}

struct StageScope {
    tip_handle* h;
    hipStream_t s;
    hipEvent_t stop = nullptr;
    StageScope(tip_handle* hh, hipStream_t ss, const char* name) : h(hh), s(ss) {
        if (!h->profile) return;
        if (h->profile >= 2 && !stage_is_dominant(name)) return;
        // 3: every FOURTH forward only — an event pair is two barrier packets in the queue, ~7 us per step at B = 256 (0.624 vs 0.631 ms,
        // measured), which a timed region should not carry on every launch
        if (h->profile == 3 && (h->forward_count & 3u) != 0) return;
        StageTimer* t = nullptr;
        for (auto& x : h->timers)
            if (x.name == name) { t = &x; break; }
        if (!t) {
            h->timers.emplace_back();
            t = &h->timers.back();
            t->name = name;
        }
        if (t->used == t->pairs.size()) {
            if (t->pairs.size() >= kMaxTimerPairs) return;
            hipEvent_t a = nullptr, b = nullptr;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            t->pairs.push_back({a, b});
        }
        auto& pr = t->pairs[t->used++];
        (void)hipEventRecord(pr.first, s);
        stop = pr.second;
    }
    ~StageScope() {
        if (stop) (void)hipEventRecord(stop, s);
    }
};

}  // namespace

// y = epi(x W^T + b (+ res)) for one packed linear of the general plan: the panel GEMM on the fragment copy when the layer
// has one and the batch is big enough, else the LDS-tiled GEMM on the row-major copy
static hipError_t linear_gemm(const float* P, const tip::PackedLinear& p, const float* A, int lda, const float* res, int ldres,
                              float* C, int ldc, int M, int flags, hipStream_t s) {
    // (the panel kernel's epilogue moves 16 bytes per lane: bias / residual / output rows must be 16-byte aligned — they are for
    //  every buffer the library carves out itself)
    auto al16 = [](const void* q, int ld) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0 && (ld & 3) == 0; };
    if (p.f_off && tip::pgemm_shape_ok(M, p.N, p.K) && al16(P + p.b_off, 0) && al16(C, ldc) && (!(flags & 2) || al16(res, ldres)))
        return tip::launch_pgemm(A, lda, P + p.f_off, (size_t)p.N * p.K, P + p.b_off, res, ldres, C, ldc, M, p.N, p.K, flags, s);
    return tip::launch_gemm(A, lda, P + p.w_off, p.Kpad, P + p.b_off, res, ldres, C, ldc, M, p.N, p.Npad, flags, s);
}

namespace tip {
namespace {
struct DevSerialState {
    std::mutex mu;
    hipStream_t last = nullptr;
    bool have = false;
    hipEvent_t ev = nullptr;
};
DevSerialState g_serial[kMaxDevices];
}  // namespace

CoopSerial::CoopSerial(int device, hipStream_t s)
    : dev(device >= 0 && device < kMaxDevices ? device : tip_cur_device()), stream(s), capturing(stream_is_capturing(s)), status(hipSuccess) {
    DevSerialState& st = g_serial[dev];
    st.mu.lock();
    if (capturing) return;   // see stream_is_capturing (tip_internal.h)
    // The event is recorded at the END of every forward (destructor), on the stream that forward ran on — known to be alive then.  A
    // stream switch therefore only waits on the event: it never touches the previous stream's handle, which may have been destroyed
    // (or recycled) by now (hipEventRecord on a dangling hipStream_t is undefined behaviour), and it cannot pull this
    // stream into another stream's capture.
    if (st.have && st.last != s && st.ev) status = hipStreamWaitEvent(s, st.ev, 0);
}

CoopSerial::~CoopSerial() {
    DevSerialState& st = g_serial[dev];
    if (!capturing) {
        if (!st.ev && hipEventCreateWithFlags(&st.ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            st.ev = nullptr;
        }
        if (st.ev) (void)hipEventRecord(st.ev, stream);
        st.last = stream;
        st.have = true;
    }
    st.mu.unlock();
}
}  // namespace tip

extern "C" {

int tip_abi_version(void) { return TIP_ABI_VERSION; }

const char* tip_strerror(int status) {
    const int i = -status;
    if (i < 0 || i >= (int)(sizeof(kStatusText) / sizeof(kStatusText[0]))) return "unknown status";
    return kStatusText[i];
}

int tip_create(const tip_config* cfg, tip_handle** out) {
    if (!cfg || !out) return TIP_ERR_INVALID_ARG;
    *out = nullptr;
    Dims d{};
    d.n_imu_total = cfg->input_size_imu + (cfg->with_acc_sum ? 18 : 0);  // simple_transformer_with_state.py:20-24
    d.S = cfg->size_s;
    d.In = d.n_imu_total + d.S;
    d.InPad = round_up(d.In, kGemmBK);
    d.D = cfg->tf_in_dim;
    d.H = cfg->n_heads;
    d.F = cfg->tf_hid_size;
    d.L = cfg->tf_layers;
    d.R = cfg->with_rnn ? cfg->rnn_hid_size : 0;
    d.with_rnn = cfg->with_rnn ? 1 : 0;
    d.t_max = cfg->t_max > 0 ? cfg->t_max : 40;
    d.rootv0 = 18 * 6;       // :75
    d.rootv1 = 18 * 6 + 3;
    if (cfg->input_size_imu <= 0 || d.S <= 0 || d.D <= 0 || d.H <= 0 || d.F <= 0 || d.L < 0) return TIP_ERR_INVALID_ARG;
    if (d.D % d.H) return TIP_ERR_INVALID_ARG;  // nn.MultiheadAttention asserts the same
    d.dh = d.D / d.H;
    if (d.D % 16 || d.F % 16 || (d.with_rnn && (d.R % 64)) ||
        !(d.dh == 8 || d.dh == 16 || d.dh == 32 || d.dh == 64) || d.D > 2048 || d.S < d.rootv1)
        return TIP_ERR_UNSUPPORTED_CONFIG;
    if (d.with_rnn && ((d.R / 16) + 3) / 4 > 8) return TIP_ERR_UNSUPPORTED_CONFIG;
    // 1/sqrt(dh) is a power of two for dh in {16, 64}: fold it into W_q / b_q exactly
    const float sc = 1.0f / sqrtf((float)d.dh);
    d.fold_q_scale = (d.dh == 16 || d.dh == 64) ? 1 : 0;
    d.q_scale = d.fold_q_scale ? 1.0f : sc;

    tip_handle* h = new (std::nothrow) tip_handle();
    if (!h) return TIP_ERR_ALLOC;
    h->cfg = *cfg;
    h->d = d;
    build_tensor_table(h);
    build_layout(h);
    h->fuse_head = 0;   // TIP_OPT_FUSE_HEAD: reserved (accepted, no effect)
    {
        // base of the dataflow launches' epoch stamps: different per handle and per process start, so that flag words another handle
        // (or an earlier life of the same address) left in a caller's workspace never read as this handle's (48 bits of splitmix64)
        static std::atomic<unsigned long long> serial{0};
        unsigned long long z = (unsigned long long)reinterpret_cast<uintptr_t>(h) ^ (serial.fetch_add(1) << 40) ^
                               (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count();
        z += 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
        h->flow_epoch = z & 0x0000ffffffffffffull;
    }
    int dev = -1;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0) {
        h->device = dev;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            h->num_cus = prop.multiProcessorCount;
        // the hand-off error word: pinned host memory the kernels can store to and the host can read without a sync
        void* hp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess && hp) {
            memset(hp, 0, 64);
            void* dp = nullptr;
            if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess && dp) {
                h->err_host = static_cast<unsigned*>(hp);
                h->err_dev = static_cast<unsigned*>(dp);
            } else {
                (void)hipHostFree(hp);
            }
        }
        (void)hipGetLastError();
    } else {
        (void)hipGetLastError();
    }
    *out = h;
    return TIP_OK;
}

void tip_destroy(tip_handle* h) {
    if (!h) return;
    for (auto& t : h->timers)
        for (auto& pr : t.pairs) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
    if (h->err_host) (void)hipHostFree(h->err_host);
    delete h;
}

const char* tip_last_hip_error(const tip_handle* h) { return h ? h->last_hip_error.c_str() : ""; }

int tip_set_option(tip_handle* h, int option, int value) {
    if (!h) return TIP_ERR_INVALID_ARG;
    switch (option) {
        case TIP_OPT_PLAN:
            if (value < TIP_PLAN_AUTO || value > TIP_PLAN_FUSED1S || value == 9 /* reserved */) return TIP_ERR_INVALID_ARG;
            if (value == 5 || value == 7 || value == 8) return TIP_ERR_UNSUPPORTED_CONFIG;   // retired plans (ABI 4): pair-split, split-fp16
            h->plan = value;
            return TIP_OK;
        case TIP_OPT_PROFILE:
            if (value < 0 || value > 3) return TIP_ERR_INVALID_ARG;
            h->profile = value;
            for (auto& t : h->timers) t.used = 0;  // reset the accumulators
            return TIP_OK;
        case TIP_OPT_RNN_CLUSTER:
            if (!(value == 0 || value == 1 || value == 2 || value == 4 || value == 8 || value == 16 || value == 32 || value == TIP_RNN_CLUSTER_ROWS4))
                return TIP_ERR_INVALID_ARG;
            h->rnn_cluster = value;
            return TIP_OK;
        case TIP_OPT_FAULT_INJECT:
            if (value < 0 || value > 31) return TIP_ERR_INVALID_ARG;
            h->fault_inject = value;
            return TIP_OK;
        case TIP_OPT_FUSE_HEAD:
            if (value < 0 || value > 1) return TIP_ERR_INVALID_ARG;
            h->fuse_head = value;
            return TIP_OK;
        case TIP_OPT_AUTO_DEMOTE:
            if (value < 0 || value > 1) return TIP_ERR_INVALID_ARG;
            h->auto_demote = value;
            return TIP_OK;
        case TIP_OPT_DEMOTED:
            if (value < 0 || value > 1) return TIP_ERR_INVALID_ARG;
            h->demoted = value;
            return TIP_OK;
        case TIP_OPT_F1S_PARTS:
            if (value != 0 && value != 2 && value != 4) return TIP_ERR_INVALID_ARG;
            h->f1s_parts = value;
            return TIP_OK;
        case TIP_OPT_NO_FLOW:
            if (value < 0 || value > 1) return TIP_ERR_INVALID_ARG;
            h->no_flow = value;
            return TIP_OK;
        case TIP_OPT_NO_ROUND_LAUNCH:
            if (value < 0 || value > 1) return TIP_ERR_INVALID_ARG;
            h->no_round_launch = value;
            return TIP_OK;
        default: return TIP_ERR_INVALID_ARG;
    }
}

int tip_check(tip_handle* h, int clear) {
    if (!h) return TIP_ERR_INVALID_ARG;
    if (!h->err_host) return TIP_OK;
    volatile unsigned* w = const_cast<volatile unsigned*>(h->err_host);
    const unsigned v = w[0] | w[1];
    if (clear) w[0] = w[1] = 0u;
    return v ? TIP_ERR_HANDOFF : TIP_OK;
}

int tip_get_option(const tip_handle* h, int option, int* value) {
    if (!h || !value) return TIP_ERR_INVALID_ARG;
    switch (option) {
        case TIP_OPT_PLAN: *value = h->plan; return TIP_OK;
        case TIP_OPT_PROFILE: *value = h->profile; return TIP_OK;
        case TIP_OPT_RNN_CLUSTER: *value = h->rnn_cluster; return TIP_OK;
        case TIP_OPT_FAULT_INJECT: *value = h->fault_inject; return TIP_OK;
        case TIP_OPT_FUSE_HEAD: *value = h->fuse_head; return TIP_OK;
        case TIP_OPT_AUTO_DEMOTE: *value = h->auto_demote; return TIP_OK;
        case TIP_OPT_DEMOTED: *value = h->demoted; return TIP_OK;
        case TIP_OPT_F1S_PARTS: *value = h->f1s_parts; return TIP_OK;
        case TIP_OPT_NO_FLOW: *value = h->no_flow; return TIP_OK;
        case TIP_OPT_NO_ROUND_LAUNCH: *value = h->no_round_launch; return TIP_OK;
        case TIP_OPT_HANDOFF_KIND: {
            const volatile unsigned* w = const_cast<const volatile unsigned*>(h->err_host);
            *value = !w ? 0 : w[0] ? 1 : w[1] ? 2 : 0;
            return TIP_OK;
        }
        default: return TIP_ERR_INVALID_ARG;
    }
}

int tip_num_tensors(const tip_handle* h) { return h ? (int)h->tensor_names.size() : TIP_ERR_INVALID_ARG; }

int tip_tensor_info(const tip_handle* h, int i, const char** name, int* rows, int* cols) {
    if (!h || i < 0 || i >= (int)h->tensor_names.size()) return TIP_ERR_INVALID_ARG;
    if (name) *name = h->tensor_names[i].c_str();
    if (rows) *rows = h->tensor_shapes[i].first;
    if (cols) *cols = h->tensor_shapes[i].second;
    return TIP_OK;
}

int tip_packed_bytes(const tip_handle* h, size_t* bytes) {
    if (!h || !bytes) return TIP_ERR_INVALID_ARG;
    *bytes = h->lay.total_floats * sizeof(float);
    return TIP_OK;
}

// The packed image from host tensors into host memory, and from device tensors into device memory (`packed_dev` is then ready for
// tip_attach_packed): one description of the image, two interpreters of it (tip_pack.hip)
int tip_pack_weights(const tip_handle* h, const float* const* t, int n, void* packed_host_out, size_t bytes) {
    return pack_weights_host(h, t, n, packed_host_out, bytes);
}

int tip_pack_weights_device(const tip_handle* h, const float* const* t, int n, void* packed_dev, size_t bytes, void* stream) {
    return pack_weights_device(h, t, n, packed_dev, bytes, static_cast<hipStream_t>(stream));
}

int tip_attach_packed(tip_handle* h, const void* packed_device, size_t bytes) {
    if (!h || !packed_device) return TIP_ERR_INVALID_ARG;
    if (bytes < h->lay.total_floats * sizeof(float)) return TIP_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(packed_device) % 256) return TIP_ERR_INVALID_ARG;
    h->packed_dev = static_cast<const float*>(packed_device);
    return TIP_OK;
}

int tip_workspace_bytes(const tip_handle* h, int B, int T, size_t* bytes) {
    if (!h || !bytes || B < 0 || T < 1) return TIP_ERR_INVALID_ARG;
    *bytes = carve_workspace(h->d, B, T).total_bytes + 256;
    return TIP_OK;
}

int tip_max_batch(const tip_handle* h, int T, int fp64, int* max_batch) {
    if (!h || !max_batch || T < 1) return TIP_ERR_INVALID_ARG;
    const Dims& d = h->d;
    long long m;
    if (fp64) {
        // tip_forward_f64: element offsets of the widest activation and of the attention grid in 32 bits; 64-row GEMM tiles on grid.y
        const long long widest = 3 * d.D > d.F ? 3 * d.D : d.F;
        m = 0x7fffffffLL / (widest * T);
        m = std::min(m, 0x7fffffffLL / ((long long)T * d.H));
        m = std::min(m, 65535LL * 64 / T);
    } else {
        // tip_forward: byte offsets of the widest activation row block through 32-bit buffer descriptors
        const long long widest = std::max(std::max(3 * d.D, d.F), std::max(d.R, d.InPad));
        m = 0x7fffffffLL / (4 * widest * T);
    }
    *max_batch = (int)std::min<long long>(m, 0x7fffffff);
    return TIP_OK;
}

int tip_forward_count(const tip_handle* h, uint64_t* n) {
    if (!h || !n) return TIP_ERR_INVALID_ARG;
    *n = h->forward_count;
    return TIP_OK;
}

int tip_profile_read(tip_handle* h, const char** names, float* ms, int* launches, int cap) {
    if (!h || cap < 0) return TIP_ERR_INVALID_ARG;
    int n = 0;
    for (auto& t : h->timers) {
        if (!t.used) continue;
        if (n < cap) {
            double total = 0.0;
            for (size_t i = 0; i < t.used; ++i) {
                float v = 0.f;
                hipError_t e = hipEventElapsedTime(&v, t.pairs[i].first, t.pairs[i].second);
                if (e != hipSuccess) return fail_hip(h, e, "hipEventElapsedTime");
                total += v;
            }
            if (names) names[n] = t.name.c_str();
            if (ms) ms[n] = (float)total;
            if (launches) launches[n] = (int)t.used;
            ++n;
        }
    }
    return n;
}

int tip_spin_timeouts(unsigned* count) {
    if (!count) return TIP_ERR_INVALID_ARG;
    unsigned a = 0, b = 0, c = 0, r = 0;
    if (read_spin_timeouts_general(&a) != hipSuccess || read_spin_timeouts_latency(&b) != hipSuccess ||
        read_spin_timeouts_fused2(&c) != hipSuccess || read_spin_timeouts_round(&r) != hipSuccess)
        return TIP_ERR_HIP;
    *count = a + b + c + r;
    return TIP_OK;
}

// The ring of tip_forward_reuse, when the forward below is that entry point's (null: tip_forward)
struct ReuseCtx {
    float* cache;
    const int* frame_ctr;
    int frame_idx;
};
// One launch sequence of a forward: the encoder of one or two parts of `n` consecutive windows, then ONE tail — the RNN input GEMM where
// the encoder did not emit it, the recurrence, the output projection — over all n.  Pointers are at the sequence's first window; the
// workspace is carved for n windows.
struct LaunchSeq {
    tip_handle* h;
    hipStream_t s;
    int cus;
    const float* x_imu;
    const float* x_s;
    const float* mask;          // null: no keep mask from the caller
    float keep_scale;
    float* y;
    const int* rows;
    int n, T, flags;
    float* W0;
    Workspace ws;
    int rnn_cluster;
    const ReuseCtx* reuse;      // full windows: the two-window encoder reads the ring
    const TrainDropout* td;     // tip_forward_dropout: the latency plan's dropout sites
    const LiveTrain* live = nullptr;   // tip_forward_live off the latency plan: the hybrid encoder runs in its live mode
    // what the encoder leaves for the tail
    int plan = TIP_PLAN_AUTO;
    bool ih_done = false;       // the RNN input projection is in `big` already
    bool hall_armed = false;    // ... and the HALL rows are pre-filled for the sentinel-polling recurrence
    bool rnn_done = false, head_done = false;
    bool round_launch = false;  // in: one round on the hybrid encoder may run as ONE launch (Schedule::round_launch and nothing of this call against it)
};

#define TIP_TRY(expr, what)                                     \
    do {                                                        \
        const hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) return fail_hip(q.h, e_, what);   \
    } while (0)
// one launch that is a profile stage of its own (tip_profile_read)
#define TIP_STAGE(name, expr)              \
    do {                                   \
        StageScope stage_(q.h, q.s, name); \
        TIP_TRY(expr, name);               \
    } while (0)

// One round on the hybrid encoder as ONE launch (tip_round.hip): encoder, recurrence and — at T = 40, where the register-resident
// projection serves — the output projection.  1: launched; a status < 0: failed; 0: the launch would not be co-resident (or the shape is
// not the form's): the caller launches the three kernels.
static int launch_round(LaunchSeq& q, const float* x_imu, const float* x_s, const float* mask, float* ih, float* hall) {
    tip_handle* h = q.h;
    const Dims& d = h->d;
    const float* P = h->packed_dev;
    const PackedLayout& L = h->lay;
    const bool last_only = (q.flags & TIP_FWD_LAST_ROW_ONLY) != 0;
    const int head = q.T == 40 && measure_switches().head_ksplit ? (last_only ? 2 : 1) : 0;
    // TIP_OPT_PROFILE = 2 / 3: the dominant stage is the launch that holds the encoder — here the whole round, recurrence and
    // projection phases included (alternating with three launches on the timed forwards was measured 3 % slower than either form)
    StageScope sc(h, q.s, "fused_encoder");
    const hipError_t e = launch_forward_round(d, P + L.fused_off, x_imu, x_s, mask, q.keep_scale, ih, hall,
                                              reinterpret_cast<unsigned*>(q.W0 + q.ws.flags), P + L.whh_frag_off, P + L.out_frag_off,
                                              P + L.out_lin.b_off, q.y, q.n, q.T, head, q.cus, h->guard(), q.s);
    if (e == hipErrorCooperativeLaunchTooLarge || e == hipErrorInvalidValue) {
        (void)hipGetLastError();
        return 0;
    }
    if (e != hipSuccess) return fail_hip(h, e, "forward_round");
    q.ih_done = q.hall_armed = q.rnn_done = true;
    q.head_done = head != 0;
    return 1;
}

// The encoder of windows [off, off + p.count) of the sequence.  (A sequence of two parts is the shared tail's: both parts are on plans
// that emit the RNN input term — only those write at a window offset.)
static int run_encoder(LaunchSeq& q, const SchedPart& p, int off) {
    tip_handle* h = q.h;
    const Dims& d = h->d;
    const float* P = h->packed_dev;
    const PackedLayout& L = h->lay;
    hipStream_t s = q.s;
    const int B = p.count, T = q.T, cus = q.cus, M = B * T;
    const size_t row_i = (size_t)T * d.n_imu_total, row_s = (size_t)T * d.S, row_r = (size_t)T * d.R;
    const float* x_imu = q.x_imu + off * row_i;
    const float* x_s = q.x_s + off * row_s;
    const float* mask = q.mask ? q.mask + off * row_s : nullptr;
    const float keep_scale = q.keep_scale;
    float* xa = q.W0 + q.ws.xa;
    float* xb = q.W0 + q.ws.xb;
    float* big = q.W0 + q.ws.big;
    float* att = q.W0 + q.ws.att;
    float* ih = big + off * row_r;
    float* hall = q.W0 + q.ws.hall + off * row_r;
    const Guard gd = h->guard();
    auto arm_hall = [&]() { return rnn_uses_sentinel(d, q.n, T, q.rnn_cluster); };
    q.plan = p.plan;
    int round_st = 0;
    if (p.plan == TIP_PLAN_LATENCY) {
        StageScope sc(h, s, "latency_chain");
        LatencyHead lh{P + L.out_frag_off, P + L.out_lin.b_off, q.y, d.S, d.S, (q.flags & TIP_FWD_LAST_ROW_ONLY) != 0, h->flow_epoch, &q.head_done,
                       reinterpret_cast<unsigned long long*>(q.W0 + q.ws.flow)};
        lh.rows = q.rows;
        TIP_TRY(launch_latency_plan(d, P + L.fused_off, P + L.whh_frag_off, x_imu, x_s, mask, keep_scale, q.W0 + q.ws.lat, hall,
                                    B, T, cus, gd, s, q.td, cus == h->num_cus && !h->no_flow ? &lh : nullptr), "latency_chain");
        q.rnn_done = true;
    } else if (p.plan == TIP_PLAN_FUSED1S) {
        StageScope sc(h, s, "fused_encoder");
        q.ih_done = true;
        q.hall_armed = arm_hall();
        TIP_TRY(launch_fused_encoder1s(d, P + L.fused_off, x_imu, x_s, mask, keep_scale, ih, q.hall_armed ? hall : nullptr,
                                       q.W0 + q.ws.xchg, B, cus, h->f1s_parts, gd, s), "fused_encoder1s");
    } else if (p.plan == TIP_PLAN_FUSED2) {
        StageScope sc(h, s, "fused_encoder");
        q.ih_done = true;
        q.hall_armed = arm_hall();
        TIP_TRY(launch_fused_encoder2(d, P + L.fused_off, x_imu, x_s, mask, keep_scale, ih, q.hall_armed ? hall : nullptr, B,
                                      cus, s, q.reuse ? q.reuse->cache : nullptr, q.reuse ? q.reuse->frame_ctr : nullptr,
                                      q.reuse ? q.reuse->frame_idx : 0), "fused_encoder2");
    } else if (p.plan == TIP_PLAN_FUSEDH && q.round_launch && (round_st = launch_round(q, x_imu, x_s, mask, ih, hall)) != 0) {
        if (round_st < 0) return round_st;
    } else if (p.plan == TIP_PLAN_FUSEDH || p.plan == TIP_PLAN_FUSED) {
        StageScope sc(h, s, "fused_encoder");
        q.ih_done = fused_has_rnn_ih(d);
        q.hall_armed = q.ih_done && arm_hall();   // the encoder pre-fills its HALL rows
        if (p.plan == TIP_PLAN_FUSEDH && q.live)
            TIP_TRY(launch_fused_live_h(d, P + L.fused_off, x_imu, x_s, mask, keep_scale, q.ih_done ? nullptr : xa, q.ih_done ? ih : nullptr,
                                        q.hall_armed ? hall : nullptr, *q.live, q.live->lv, B, T, cus, s), "fused_encoder_h live");
        else if (p.plan == TIP_PLAN_FUSEDH)
            TIP_TRY(launch_fused_encoder_h(d, P + L.fused_off, x_imu, x_s, mask, keep_scale, q.ih_done ? nullptr : xa,
                                           q.ih_done ? ih : nullptr, q.hall_armed ? hall : nullptr, B, T, cus, s), "fused_encoder_h");
        else
            TIP_TRY(launch_fused_encoder(d, P + L.fused_off, x_imu, x_s, mask, keep_scale, q.ih_done ? nullptr : xa,
                                         q.ih_done ? ih : nullptr, q.hall_armed ? hall : nullptr, B, T, cus, s), "fused_encoder");
    } else {
        TIP_STAGE("prologue", launch_prologue(d, x_imu, x_s, mask, keep_scale, big, M, s));
        TIP_STAGE("in_linear", launch_gemm(big, d.InPad, P + L.in_lin.w_off, L.in_lin.Kpad, P + L.in_lin.b_off, nullptr, 0, xa,
                                             d.D, M, d.D, L.in_lin.Npad, 0, s));
        for (int l = 0; l < d.L; ++l) {
            const PackedLayer& pl = L.layers[l];
            TIP_STAGE("qkv_gemm", linear_gemm(P, pl.qkv, xa, d.D, nullptr, 0, big, 3 * d.D, M, 0, s));
            TIP_STAGE("attention", launch_attention(d, big, att, B, T, s));
            TIP_STAGE("out_proj_gemm", linear_gemm(P, pl.out, att, d.D, xa, d.D, xb, d.D, M, 2, s));
            TIP_STAGE("layernorm1", launch_layernorm(xb, P + pl.g1_off, P + pl.be1_off, M, d.D, s));
            TIP_STAGE("ffn1_gemm", linear_gemm(P, pl.ff1, xb, d.D, nullptr, 0, big, d.F, M, 1, s));
            TIP_STAGE("ffn2_gemm", linear_gemm(P, pl.ff2, big, d.F, xb, d.D, xa, d.D, M, 2, s));
            TIP_STAGE("layernorm2", launch_layernorm(xa, P + pl.g2_off, P + pl.be2_off, M, d.D, s));
        }
    }
    return TIP_OK;
}

// RNN input GEMM (where the encoder left the plain rows in xa), recurrence, output projection — over all q.n windows
static int run_tail(LaunchSeq& q) {
    tip_handle* h = q.h;
    const Dims& d = h->d;
    const float* P = h->packed_dev;
    const PackedLayout& L = h->lay;
    hipStream_t s = q.s;
    const int B = q.n, T = q.T, M = B * T;
    float* big = q.W0 + q.ws.big;
    float* hall = q.W0 + q.ws.hall;
    const float* head_in = q.W0 + q.ws.xa;   // encoder output [M, D]
    int head_ld = d.D;
    if (d.with_rnn) {
        if (!q.rnn_done && !q.ih_done)
            TIP_STAGE("rnn_ih_gemm", launch_gemm(head_in, d.D, P + L.rnn_ih.w_off, L.rnn_ih.Kpad, P + L.rnn_ih.b_off, nullptr, 0, big, d.R, M, d.R,
                                                 L.rnn_ih.Npad, 0, s));
        if (!q.rnn_done)
            TIP_STAGE("rnn_recurrence", launch_rnn(d, big, P + L.whh_frag_off, hall, reinterpret_cast<unsigned*>(q.W0 + q.ws.flags), B, T,
                                                   q.rnn_cluster, q.cus, q.hall_armed, h->guard(), s));
        head_in = hall;
        head_ld = d.R;
    }
    if (!q.head_done) {
        StageScope sc(h, s, "out_linear");
        const bool last_only = (q.flags & TIP_FWD_LAST_ROW_ONLY) != 0;
        const int* rows = q.rows;
        const int Kh = d.with_rnn ? d.R : d.D;
        // rows the projection runs on: all M, or row T-1 of every window (real_time_runner_minimal.py:150), or row rows[b] of window b
        // (tip_forward_rows: A is then the first row, lda the row stride)
        const float* hA = last_only && !rows ? head_in + (size_t)(T - 1) * head_ld : head_in;
        const long long hlda = last_only && !rows ? (long long)T * head_ld : head_ld;
        const int hM = last_only ? B : M;
        if (q.plan == TIP_PLAN_LATENCY) {
            TIP_TRY(launch_latency_head(hA, hlda, P + L.out_frag_off, P + L.out_lin.b_off, q.y, d.S, hM, d.S, s, rows, T), "out_linear");
        } else {
            // window lengths that are multiples of 40 (the paper's and the scaled configuration's): the register-resident
            // kernel for both forms of the output (bit-identical last rows); everything else: head_gemm_kernel for both
            hipError_t he = hipErrorInvalidValue;
            if (measure_switches().head_ksplit && T % 40 == 0)   // TIP_HEAD=old: measurement
                he = launch_head_ksplit(hA, hlda, P + L.out_frag_off, P + L.out_lin.b_off, q.y, d.S, hM, d.S, Kh, last_only, q.cus, s, rows, T);
            if (he == hipErrorInvalidValue)
                he = launch_head_gemm(hA, hlda, P + L.out_frag_off, P + L.out_lin.b_off, q.y, d.S, hM, d.S, Kh, s, rows, T);
            TIP_TRY(he, "out_linear");
        }
    }
    return TIP_OK;
}
#undef TIP_STAGE
#undef TIP_TRY

// What every forward entry point settles before its first launch (forward_prepare)
struct ForwardPrep {
    hipStream_t s;
    int cus;              // the stream's CU mask counts, not the device's CU total
    Workspace ws;         // the carve-up for all B windows
    const float* mask;    // null: no keep mask from the caller
    float keep_scale;     // 1 unless a keep mask is applied — the caller's, or one drawn inside the first kernel (`mask_drawn`)
    bool few;             // the few-stream latency plan serves this call (live entry points)
};
// plans an entry point runs on: what schedule_forward picks after the preamble (tip_forward / _rows / _reuse), the few-stream latency
// plan only (tip_forward_dropout), or that plan where it serves and the hybrid encoder's live mode elsewhere (tip_forward_live)
enum ForwardServe { kServeScheduled, kServeFewOnly, kServeLive };

// The preamble of every forward entry point: argument, readiness and hand-off checks, the B == 0 exit, the entry point's plan-support
// test, the workspace, then stream and CU count.  True: go on and launch with *p.  False: return *status (TIP_OK for an empty batch).
static bool forward_prepare(tip_handle* h, const float* x_imu, const float* x_s, const float* y, int B, int T, int flags, const float* keep_mask,
                            float keep_scale, bool mask_drawn, void* workspace, size_t workspace_bytes, tip_stream_t stream,
                            ForwardServe serve, ForwardPrep* p, int* status) {
    auto stop = [&](int st) { *status = st; return false; };
    if (!h || !x_imu || !x_s || !y || B < 0 || T < 1) return stop(TIP_ERR_INVALID_ARG);
    const Dims& d = h->d;
    // (cfg.t_max is a sizing hint, not a limit: the reference builds its causal mask for any window length, :56-58,85; what
    // bounds B * T here are the 32-bit byte offsets of the buffer descriptors)
    if ((long long)B * T * (long long)std::max(std::max(3 * d.D, d.F), std::max(d.R, d.InPad)) * 4 > 0x7fffffffLL)
        return stop(TIP_ERR_UNSUPPORTED_CONFIG);
    if ((flags & TIP_FWD_KEEP_MASK) && !keep_mask) return stop(TIP_ERR_INVALID_ARG);
    if (!h->packed_dev) return stop(TIP_ERR_NOT_READY);
    if (tip_check(h, 0) != TIP_OK) return stop(TIP_ERR_HANDOFF);   // sticky: an earlier launch lost a hand-off (tip_check(h, 1) clears)
    if (B == 0) return stop(TIP_OK);
    // the few-stream latency plan is the only one with the dropout sites; a demoted handle takes no cooperating kernel (its GEMV
    // recurrence is one).  tip_forward_dropout's caller falls back to tip_train_forward; tip_forward_live runs everything else — a
    // demoted handle too — on the one-window hybrid encoder's live mode, which serves what the hybrid training forward serves
    p->few = serve != kServeScheduled && !h->demoted && latency_supported(d, B, T);
    if (serve == kServeFewOnly && !p->few) return stop(TIP_ERR_UNSUPPORTED_CONFIG);
    if (serve == kServeLive && !p->few && !(fused_supported(d, T) && fused_has_rnn_ih(d))) return stop(TIP_ERR_UNSUPPORTED_CONFIG);
    p->ws = carve_workspace(d, B, T);
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 256 || workspace_bytes < p->ws.total_bytes) return stop(TIP_ERR_WORKSPACE);
    p->s = static_cast<hipStream_t>(stream);
    p->cus = effective_cus(h->num_cus, p->s);
    p->mask = (flags & TIP_FWD_KEEP_MASK) ? keep_mask : nullptr;
    p->keep_scale = p->mask || mask_drawn ? keep_scale : 1.f;
    return true;
}

// rows (tip_forward_rows; null: tip_forward): one output row per window, row rows[b] of window b — only the output projection's row
// addressing differs (TIP_FWD_LAST_ROW_ONLY is set with it, so everything that depends on the output's shape takes the last-row form)
static int forward_impl(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, int flags,
                        const float* keep_mask, float keep_scale, void* workspace, size_t workspace_bytes,
                        tip_stream_t stream, const ReuseCtx* reuse, const int* rows = nullptr) {
    ForwardPrep f;
    int status;
    if (!forward_prepare(h, x_imu, x_s, y, B, T, flags, keep_mask, keep_scale, false, workspace, workspace_bytes, stream, kServeScheduled, &f, &status))
        return status;
    const Dims& d = h->d;
    hipStream_t s = f.s;
    // (tip_forward_reuse, full windows: ONE launch sequence on the two-window encoder's reuse form, whatever the batch; while the windows
    // still grow, T < 40, the ring update below is all the reuse form does and the forward is tip_forward's)
    const bool reuse_full = reuse && T == 40;
    const Schedule sc = schedule_forward(ScheduleIn{d, B, T, f.cus, h->num_cus, h->plan, h->rnn_cluster, h->f1s_parts, h->demoted != 0, reuse_full,
                                                    workspace_bytes, h->no_round_launch != 0});
    if (sc.status != TIP_OK) return sc.status;
    const size_t row_i = (size_t)T * d.n_imu_total, row_s = (size_t)T * d.S;
    const size_t row_y = (flags & TIP_FWD_LAST_ROW_ONLY) ? (size_t)d.S : row_s;
    // A shared tail: both parts in ONE launch sequence over the whole batch's carve-up.  Otherwise every part is a launch sequence of its
    // own, carved for its own windows from the start of the same workspace (stream-ordered).
    const int nseq = sc.shared_tail ? 1 : sc.nparts;
    for (int i = 0; i < nseq; ++i) {
        const int first = sc.part[i].first, n = sc.shared_tail ? B : sc.part[i].count;
        LaunchSeq q{h, s, f.cus, x_imu + first * row_i, x_s + first * row_s, f.mask ? f.mask + first * row_s : nullptr, f.keep_scale,
                    y + first * row_y, rows ? rows + first : nullptr, n, T, flags, static_cast<float*>(workspace),
                    n == B ? f.ws : carve_workspace(d, n, T), sc.part[i].rnn_cluster, reuse_full ? reuse : nullptr, nullptr};
        // (a stage of TIP_OPT_PROFILE = 1 is a launch: three launches then; under 2 and 3 the pair of the dominant stage brackets the
        // launch that holds the encoder, launch_round.  tip_forward_rows gathers its rows in launches of its own)
        q.round_launch = sc.round_launch && h->profile != 1 && !rows;
        CoopSerial serial(h->device, s);   // forwards of different streams do not overlap on the device (cooperating kernels)
        if (serial.status != hipSuccess) return fail_hip(h, serial.status, "stream serialisation");
        if (reuse) {
            // the newest row of every window -> slot (frame mod 40) of its stream's ring (a reuse forward is always one sequence)
            StageScope stage(h, s, "reuse_update");
            const hipError_t e = launch_reuse_update(d, h->packed_dev + h->lay.fused_off, x_imu, x_s, reuse->cache, reuse->frame_ctr, reuse->frame_idx, B, T, s);
            if (e != hipSuccess) return fail_hip(h, e, "reuse_update");
        }
        for (int p = i; p < (sc.shared_tail ? sc.nparts : i + 1); ++p) {
            const int st = run_encoder(q, sc.part[p], sc.part[p].first - first);
            if (st != TIP_OK) return st;
        }
        const int st = run_tail(q);
        if (st != TIP_OK) return st;
    }
    h->forward_count++;   // one forward, however many launch sequences
    return TIP_OK;
}

int tip_forward(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, int flags,
                const float* keep_mask, float keep_scale, void* workspace, size_t workspace_bytes,
                tip_stream_t stream) {
    return forward_impl(h, x_imu, x_s, y, B, T, flags, keep_mask, keep_scale, workspace, workspace_bytes, stream, nullptr);
}

int tip_forward_rows(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, const int* rows, int flags,
                     const float* keep_mask, float keep_scale, void* workspace, size_t workspace_bytes, tip_stream_t stream) {
    if (!rows && B > 0) return TIP_ERR_INVALID_ARG;
    return forward_impl(h, x_imu, x_s, y, B, T, flags | TIP_FWD_LAST_ROW_ONLY, keep_mask, keep_scale, workspace, workspace_bytes, stream,
                        nullptr, rows);
}

int tip_reuse_cache_bytes(const tip_handle* h, int n_streams, size_t* bytes) {
    if (!h || !bytes || n_streams < 0) return TIP_ERR_INVALID_ARG;
    if (!fused2_supported(h->d, 40)) return TIP_ERR_UNSUPPORTED_CONFIG;
    *bytes = reuse_cache_floats(n_streams) * sizeof(float);
    return TIP_OK;
}

int tip_reuse_reset(void* cache, size_t cache_bytes, tip_stream_t stream) {
    if (!cache || cache_bytes < reuse_cache_floats(0) * sizeof(float)) return TIP_ERR_INVALID_ARG;
    // every slot's tag <- INT_MIN: no frame index a caller may pass (>= 0) makes a window's 40 tags match
    return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(cache), (int)0x80000000, reuse_cache_floats(0), static_cast<hipStream_t>(stream)) == hipSuccess
               ? TIP_OK
               : TIP_ERR_HIP;
}

int tip_forward_reuse(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, int flags, void* cache,
                      size_t cache_bytes, int frame_idx, const int* frame_ctr, void* workspace, size_t workspace_bytes,
                      tip_stream_t stream) {
    if (!h || !cache || B < 0 || T < 1 || (flags & TIP_FWD_KEEP_MASK) || (!frame_ctr && frame_idx < 0)) return TIP_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(cache) % 256 || cache_bytes < reuse_cache_floats(B) * sizeof(float)) return TIP_ERR_WORKSPACE;
    if (!fused2_supported(h->d, 40) || T > 40) return TIP_ERR_UNSUPPORTED_CONFIG;
    if (T == 40 && !frame_ctr && frame_idx < 39) return TIP_ERR_INVALID_ARG;   // a full window has 39 earlier frames
    const ReuseCtx rc{static_cast<float*>(cache), frame_ctr, frame_idx};
    return forward_impl(h, x_imu, x_s, y, B, T, flags, nullptr, 1.f, workspace, workspace_bytes, stream, &rc);
}

int tip_draw_keep_mask(float p_state, unsigned long long state_seed, float* mask, size_t n, tip_stream_t stream) {
    unsigned key = 0, thresh = 0;
    if ((!mask && n) || !state_mask_params(p_state, state_seed, &key, &thresh)) return TIP_ERR_INVALID_ARG;
    return launch_keep_mask(mask, n, key, thresh, static_cast<hipStream_t>(stream)) == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

// tip_forward_dropout and tip_forward_live: ONE launch sequence with the encoder's dropout sites and the past-state keep mask live.
// few_only (tip_forward_dropout): the few-stream latency plan or TIP_ERR_UNSUPPORTED_CONFIG, never the hybrid encoder's live mode.
static int live_impl(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, const int* rows, int flags,
                     const float* keep_mask, float keep_scale, float p_state, unsigned long long state_seed, float p_drop,
                     unsigned long long seed, const unsigned long long* seeds_dev, void* workspace, size_t workspace_bytes,
                     tip_stream_t stream, bool few_only) {
    if (p_drop < 0.f || p_drop >= 1.f) return TIP_ERR_INVALID_ARG;
    if (rows) flags |= TIP_FWD_LAST_ROW_ONLY;
    unsigned mkey = 0, mthresh = 0;
    if (!(flags & TIP_FWD_KEEP_MASK) && p_state > 0.f && !state_mask_params(p_state, state_seed, &mkey, &mthresh)) return TIP_ERR_INVALID_ARG;
    ForwardPrep f;
    int status;
    if (!forward_prepare(h, x_imu, x_s, y, B, T, flags, keep_mask, keep_scale, mthresh != 0, workspace, workspace_bytes, stream,
                         few_only ? kServeFewOnly : kServeLive, &f, &status))
        return status;
    int rnn_cluster = 0;
    if (!f.few) {   // (the recurrence variant as the forward pinned to the hybrid plan resolves it)
        const Schedule sc = schedule_forward(ScheduleIn{h->d, B, T, f.cus, h->num_cus, TIP_PLAN_FUSEDH, h->rnn_cluster, h->f1s_parts, h->demoted != 0,
                                                        false, workspace_bytes});
        if (sc.status != TIP_OK) return sc.status;
        rnn_cluster = sc.part[0].rnn_cluster;
    }
    CoopSerial serial(h->device, f.s);
    if (serial.status != hipSuccess) return fail_hip(h, serial.status, "stream serialisation");
    TrainDropout td = make_train_dropout(p_drop, seed);
    td.mkey = mkey;
    td.mthresh = mthresh;
    td.seeds_dev = seeds_dev;   // (td.state_seed stays 0: the few-stream plan's mask key is mkey, the hybrid live mode reads lt.lv)
    LiveTrain lt;
    lt.sv = nullptr;
    lt.x0 = lt.qkv = lt.ast = lt.att = lt.z1 = lt.st1 = lt.x1 = lt.hid = lt.z2 = lt.st2 = lt.xo = lt.layer_stride = 0;
    lt.seed = seed; lt.thresh = td.thresh; lt.scale = td.scale;
    lt.lv = LiveArgs{seeds_dev, state_seed, f.mask ? 0u : mthresh};
    LaunchSeq q{h, f.s, f.cus, x_imu, x_s, f.mask, f.keep_scale, y, rows, B, T, flags, static_cast<float*>(workspace), f.ws, rnn_cluster, nullptr,
                f.few ? &td : nullptr, f.few ? nullptr : &lt};
    int st = run_encoder(q, SchedPart{0, B, f.few ? TIP_PLAN_LATENCY : TIP_PLAN_FUSEDH, rnn_cluster}, 0);
    if (st == TIP_OK) st = run_tail(q);
    if (st != TIP_OK) return st;
    h->forward_count++;
    return TIP_OK;
}

int tip_forward_dropout(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, int flags,
                        const float* keep_mask, float keep_scale, float p_state, unsigned long long state_seed, float p_drop,
                        unsigned long long seed, void* workspace, size_t workspace_bytes, tip_stream_t stream) {
    return live_impl(h, x_imu, x_s, y, B, T, nullptr, flags, keep_mask, keep_scale, p_state, state_seed, p_drop, seed, nullptr, workspace,
                     workspace_bytes, stream, true);
}

int tip_forward_live(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, const int* rows, int flags,
                     const float* keep_mask, float keep_scale, float p_state, unsigned long long state_seed, float p_drop,
                     unsigned long long seed, const unsigned long long* seeds_dev, void* workspace, size_t workspace_bytes,
                     tip_stream_t stream) {
    return live_impl(h, x_imu, x_s, y, B, T, rows, flags, keep_mask, keep_scale, p_state, state_seed, p_drop, seed, seeds_dev, workspace,
                     workspace_bytes, stream, false);
}

int tip_seeds_next(unsigned long long* seeds_dev, tip_stream_t stream) {
    if (!seeds_dev || reinterpret_cast<uintptr_t>(seeds_dev) % 8) return TIP_ERR_INVALID_ARG;
    return launch_seeds_next(seeds_dev, static_cast<hipStream_t>(stream)) == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

}  // extern "C"
static_assert(tip::kRnnRows4 == TIP_RNN_CLUSTER_ROWS4, "option value");
