// tip_pack.hip — everything about the packed weight image: its layout, and building it from the 56 state-dict tensors.
// The image is described ONCE, as a list of PackOps (image_pack_ops; the fused section's part is fused_pack_ops in tip_fused.hip):
// general-plan section (row-major, zero padded), W_hh / out-linear in MFMA fragment order, fused-plan section (fragment order), with
// the folds of DESIGN.md section 4 (channel shuffle :88-89 into in_linear rows, root-velocity zeroing :75 into its columns,
// 1/sqrt(d_head) into W_q, b_ih + b_hh).  One op per destination array.  Two interpreters of the list: pack_ops_kernel from device
// tensors (a handful of launches, microseconds — which is what makes `load_state_dict` / optimiser-step -> inference round trips
// cheap), the loop of run_pack_ops_host from host tensors.  What they share is the VALUE of an element, pack_row + pack_value
// (tip_internal.h); the storage order of a fragment array is decoded from the element index by the kernel and walked block by block by
// the host.
#include <math.h>
#include <string.h>

#include "tip_internal.h"

namespace tip {

__global__ __launch_bounds__(256) void pack_ops_kernel(PackBatch pb, float* __restrict__ img) {
    const PackOp& op = pb.ops[blockIdx.y];
    const long long total = (long long)op.N * op.K;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        int n, k;
        if (op.frag) {
            // i = ((nb*KB + kb)*64 + lane)*4 + s
            const int s = (int)(i & 3), lane = (int)((i >> 2) & 63);
            const long long blk = i >> 8;
            const int KB = op.K >> 4;
            const int kb = (int)(blk % KB), nb = (int)(blk / KB);
            n = nb * 16 + (lane & 15);
            k = kb * 16 + 4 * (lane >> 4) + s;
        } else {
            n = (int)(i / op.K);
            k = (int)(i - (long long)n * op.K);
        }
        img[op.dst_off + i] = pack_value(op, pack_row(op, n), k);
    }
}

hipError_t run_pack_ops(const std::vector<PackOp>& ops, float* img, hipStream_t s) {
    for (size_t o = 0; o < ops.size(); o += kPackBatch) {
        PackBatch pb;
        const int n = (int)std::min<size_t>(kPackBatch, ops.size() - o);
        long long maxel = 1;
        for (int i = 0; i < n; ++i) {
            pb.ops[i] = ops[o + i];
            maxel = std::max(maxel, (long long)ops[o + i].N * ops[o + i].K);
        }
        int gx = (int)std::min<long long>((maxel + 255) / 256, 256);
        hipLaunchKernelGGL(pack_ops_kernel, dim3(gx, n), dim3(256), 0, s, pb, img);
    }
    return hipGetLastError();
}

// The host walks ROWS in its outer loop, for both storage orders: pack_row once per row, only k in the inner loop, the source row read
// front to back.  In fragment order [N/16][K/16][64 lanes][4] element (n, k) sits in lane (n & 15) + 16 * ((k >> 2) & 3) of block
// (n >> 4, k >> 4), slot k & 3: within the 16-row strip of n that is float 4 * (n & 15) + 64 * (k >> 2) + (k & 3) (K % 16 == 0).  Decoding every
// index as the kernel does (two 64-bit divisions per element), or evaluating the row part per element, costs this loop a factor of
// about 1.5 each (CHANGELOG).  No per-op fast paths beyond that.
void run_pack_ops_host(const std::vector<PackOp>& ops, float* img) {
    for (size_t o = 0; o < ops.size(); ++o) {
        const PackOp op = ops[o];   // a copy: the stores below cannot alias its fields
        float* dst = img + op.dst_off;
        for (int n = 0; n < op.N; ++n) {
            const PackRow row = pack_row(op, n);
            if (op.frag) {
                float* d = dst + (size_t)(n >> 4) * 16 * op.K + 4 * (n & 15);
                for (int k = 0; k < op.K; k += 4, d += 64)
                    for (int s = 0; s < 4; ++s) d[s] = pack_value(op, row, k + s);
            } else {
                float* d = dst + (size_t)n * op.K;
                for (int k = 0; k < op.K; ++k) d[k] = pack_value(op, row, k);
            }
        }
    }
}

namespace {

// offsets are in floats, every section 64-float (256 B) aligned
struct Carver {
    size_t off = 0;
    size_t take(size_t n) {
        size_t o = off;
        off = (off + n + 63) / 64 * 64;
        return o;
    }
};

PackedLinear carve_linear(Carver& c, int N, int K) {
    PackedLinear p;
    p.N = N;
    p.K = K;
    p.Npad = round_up(N, kGemmBN);
    p.Kpad = round_up(K, kGemmBK);
    p.w_off = c.take((size_t)p.Npad * p.Kpad);
    p.b_off = c.take((size_t)p.Npad);
    return p;
}

// The inference image as ops: t = the 56 tensors in state-dict order (tip_tensor_info)
void image_pack_ops(const Dims& d, const PackedLayout& L, const float* const* t, std::vector<PackOp>& ops) {
    const float q_sc = 1.0f / sqrtf((float)d.dh);   // folded only where it is a power of two: exact
    auto fold_q = [&](PackOp o) {
        if (d.fold_q_scale) { o.scale = q_sc; o.scale_rows = d.D; }
        return o;
    };
    auto weight = [](const PackedLinear& p, const float* W) { return rows_op(W, p.w_off, p.Npad, p.Kpad, p.N, p.K); };
    auto bias = [](const PackedLinear& p, const float* b) { return rows_op(b, p.b_off, p.Npad, 1, p.N, 1); };
    auto linear = [&](const PackedLinear& p, const float* W, const float* b) {
        ops.push_back(weight(p, W));
        ops.push_back(bias(p, b));
    };
    {
        // in_linear with the channel shuffle (:88-89) folded into its rows and the root-velocity zeroing (:75) folded into its
        // columns: packed row a*H + b = reference row b*dh + a
        PackOp w = weight(L.in_lin, t[0]);
        w.shuffle_h = d.H; w.shuffle_dh = d.dh;
        w.z0 = d.n_imu_total + d.rootv0; w.z1 = d.n_imu_total + d.rootv1;
        ops.push_back(w);
        PackOp b = bias(L.in_lin, t[1]);
        b.shuffle_h = d.H; b.shuffle_dh = d.dh;
        ops.push_back(b);
    }
    for (int l = 0; l < d.L; ++l) {
        const float* const* lw = t + 2 + 12 * l;
        const PackedLayer& pl = L.layers[l];
        ops.push_back(fold_q(weight(pl.qkv, lw[0])));
        ops.push_back(fold_q(bias(pl.qkv, lw[1])));
        linear(pl.out, lw[2], lw[3]);
        linear(pl.ff1, lw[4], lw[5]);
        linear(pl.ff2, lw[6], lw[7]);
        // big linears also in fragment order [N/16][K/16][64 lanes][4] for the panel GEMM, with the same folds
        const PackedLinear* pls[4] = {&pl.qkv, &pl.out, &pl.ff1, &pl.ff2};
        for (int i = 0; i < 4; ++i) {
            const PackedLinear& p = *pls[i];
            if (!p.f_off) continue;
            const PackOp f = frag_op(lw[2 * i], p.f_off, p.N, p.K, p.N, p.K);
            ops.push_back(i == 0 ? fold_q(f) : f);
        }
        const size_t ln[4] = {pl.g1_off, pl.be1_off, pl.g2_off, pl.be2_off};
        for (int i = 0; i < 4; ++i) ops.push_back(rows_op(lw[8 + i], ln[i], d.D, 1, d.D, 1));
    }
    const float* const* tw = t + 2 + 12 * d.L;
    const float* Wo = tw[0];
    int Ko = d.D;
    if (d.with_rnn) {
        linear(L.rnn_ih, tw[0], tw[2]);
        ops.back().src2 = tw[3];                                           // b_ih + b_hh
        ops.push_back(frag_op(tw[1], L.whh_frag_off, d.R, d.R, d.R, d.R));
        Wo = tw[4]; Ko = d.R;
    }
    linear(L.out_lin, Wo, d.with_rnn ? tw[5] : tw[1]);
    ops.push_back(frag_op(Wo, L.out_frag_off, round_up(d.S, 16), Ko, d.S, Ko));   // for the skinny head GEMM
    if (L.fused_floats) fused_pack_ops(d, t, L.fused_off, ops);
}

bool pack_args_ok(const tip_handle* h, const float* const* t, int n, const void* out, size_t bytes) {
    if (!h || !t || !out) return false;
    if (n != (int)h->tensor_names.size()) return false;
    if (bytes < h->lay.total_floats * sizeof(float)) return false;
    for (int i = 0; i < n; ++i)
        if (!t[i]) return false;
    return true;
}

}  // namespace

void build_layout(tip_handle* h) {
    const Dims& d = h->d;
    Carver c;
    PackedLayout& L = h->lay;
    L.in_lin = carve_linear(c, d.D, d.In);
    L.layers.assign(d.L, PackedLayer{});
    for (int l = 0; l < d.L; ++l) {
        PackedLayer& pl = L.layers[l];
        pl.qkv = carve_linear(c, 3 * d.D, d.D);
        pl.out = carve_linear(c, d.D, d.D);
        pl.ff1 = carve_linear(c, d.F, d.D);
        pl.ff2 = carve_linear(c, d.D, d.F);
        pl.g1_off = c.take(d.D);
        pl.be1_off = c.take(d.D);
        pl.g2_off = c.take(d.D);
        pl.be2_off = c.take(d.D);
        // big linears also in MFMA fragment order for the panel GEMM (tip_fused2.hip, launch_pgemm)
        for (PackedLinear* p : {&pl.qkv, &pl.out, &pl.ff1, &pl.ff2})
            if (pgemm_shape_ok(1 << 20, p->N, p->K)) p->f_off = c.take((size_t)p->N * p->K);
    }
    if (d.with_rnn) {
        L.rnn_ih = carve_linear(c, d.R, d.D);
        L.whh_frag_off = c.take((size_t)d.R * d.R);
        L.out_lin = carve_linear(c, d.S, d.R);
        L.out_frag_off = c.take((size_t)round_up(d.S, 16) * d.R);
    } else {
        L.rnn_ih = PackedLinear{};
        L.whh_frag_off = 0;
        L.out_lin = carve_linear(c, d.S, d.D);
        L.out_frag_off = c.take((size_t)round_up(d.S, 16) * d.D);
    }
    L.fused_floats = fused_packed_floats(d);
    L.fused_off = c.take(L.fused_floats);
    L.total_floats = c.off;
}

int pack_weights_host(const tip_handle* h, const float* const* t, int n, void* packed_host_out, size_t bytes) {
    if (!pack_args_ok(h, t, n, packed_host_out, bytes)) return TIP_ERR_INVALID_ARG;
    std::vector<PackOp> ops;
    image_pack_ops(h->d, h->lay, t, ops);
    memset(packed_host_out, 0, h->lay.total_floats * sizeof(float));
    run_pack_ops_host(ops, static_cast<float*>(packed_host_out));
    return TIP_OK;
}

int pack_weights_device(const tip_handle* h, const float* const* t, int n, void* packed_dev, size_t bytes, hipStream_t s) {
    if (!pack_args_ok(h, t, n, packed_dev, bytes)) return TIP_ERR_INVALID_ARG;
    std::vector<PackOp> ops;
    image_pack_ops(h->d, h->lay, t, ops);
    if (hipMemsetAsync(packed_dev, 0, h->lay.total_floats * sizeof(float), s) != hipSuccess) return TIP_ERR_HIP;
    if (run_pack_ops(ops, static_cast<float*>(packed_dev), s) != hipSuccess) return TIP_ERR_HIP;
    return TIP_OK;
}

}  // namespace tip
