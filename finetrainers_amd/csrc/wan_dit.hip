// Wan-T2V DiT block for FULL fine-tuning (and, below, for LoRA fine-tuning over a frozen base), forward / backward orchestrator: ONE C call per block and direction -- the unit FSDP-2 shards
// (finetrainers/parallel/ptd.py:466-499 wraps every block with fully_shard), so the sharder keeps interleaving its all-gathers and reduce-scatters
// between the calls.  Parameters arrive as the block's ONE flat bf16 buffer, gradients leave in ONE flat fp32 buffer of the same layout
// (finetrainers_amd/wan/block.py WanBlockLayout; the order is restated in Offsets below), activations live in a caller-owned `saved` buffer per
// block (every one of them is read again: all parameters train) and transients in a `scratch` buffer shared by all blocks.
//
//   x [B, S, D] video tokens, enc [B, T, D] text tokens, mod fp32 [B, 6, D] = scale_shift_table + time projection (shift, scale, gate) x 2:
//     n1 = LN(x) * (1 + scale_msa) + shift_msa;  q|k|v = n1 W^T + b;  q, k <- RMSNorm across heads, rotary embedding;  o1 = attention(q, k, v)
//     x1 = x + gate_msa * (o1 W_o^T + b)
//     n2 = LN(x1; norm2);  q2 = n2 W^T + b;  k2|v2 = enc W^T + b;  q2, k2 <- RMSNorm;  o2 = attention(q2, k2, v2);  x2 = x1 + (o2 W_o2^T + b)
//     n3 = LN(x2) * (1 + scale_ff) + shift_ff;  out = x2 + gate_ff * (gelu_tanh(n3 W_1^T + b) W_2^T + b)
//
// Reference: [upstream] diffusers WanTransformerBlock / WanAttnProcessor2_0 as driven by finetrainers/models/wan/base_specification.py:433-493,
// restated in oracle/wan.py.  The kernel sequence is the one finetrainers_amd/wan/block.py (_WanBlockFunction) issues from Python, which stays as the
// second implementation (the tests compare the two bit for bit, parameter gradients up to the order of their fp32 atomics).
#include "common.hip.h"
#include "kernels.h"

namespace ftmi {

namespace {

struct Bump {
    size_t off = 0;
    size_t take(size_t bytes) {
        size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

// element offsets of the parameters inside a block's flat buffer (WanBlockLayout.entries, same order)
struct Offsets {
    size_t w_qkv1, b_qkv1, w_o1, b_o1, nq1, nk1, w_q2, b_q2, w_kv2, b_kv2, w_o2, b_o2, nq2, nk2, n2w, n2b, w_f1, b_f1, w_f2, b_f2, table, total;
};
Offsets offsets_of(size_t D, size_t F) {
    Offsets o;
    size_t p = 0;
    o.w_qkv1 = p; p += 3 * D * D;   // attn1.to_q / to_k / to_v .weight
    o.b_qkv1 = p; p += 3 * D;       // their biases
    o.w_o1 = p; p += D * D;
    o.b_o1 = p; p += D;
    o.nq1 = p; p += D;
    o.nk1 = p; p += D;
    o.w_q2 = p; p += D * D;
    o.b_q2 = p; p += D;
    o.w_kv2 = p; p += 2 * D * D;    // attn2.to_k / to_v .weight
    o.b_kv2 = p; p += 2 * D;
    o.w_o2 = p; p += D * D;
    o.b_o2 = p; p += D;
    o.nq2 = p; p += D;
    o.nk2 = p; p += D;
    o.n2w = p; p += D;
    o.n2b = p; p += D;
    o.w_f1 = p; p += F * D;
    o.b_f1 = p; p += F;
    o.w_f2 = p; p += D * F;
    o.b_f2 = p; p += D;
    o.table = p; p += 6 * D;
    o.total = p;
    return o;
}

struct WanLayout {
    // saved
    size_t n1, qkv, qn, kn, o1, lse1, a1, x1, n2, q2, kv2, q2n, k2n, o2, lse2, x2, n3, act, pre, f, saved_total;
    // scratch (backward)
    size_t t_f2, t_f1, t_o2, t_q2, t_kv2, t_o1, t_qkv1;                      // transposed weights
    size_t df, dpre, dn3, dx2, do2, dkv2, dq2n, dk2n, dq2, dn2, dx1, da1, do1, dqkv, dqn, dkn, dn1, delta, scratch_total;
};

WanLayout make_layout(const ftmi_wan_block_config& c) {
    WanLayout w;
    const size_t M = (size_t)c.B * c.S, Mt = (size_t)c.B * c.T, D = c.D, F = c.F, e2 = 2;
    Bump s;
    w.n1 = s.take(M * D * e2);
    w.qkv = s.take(M * 3 * D * e2);
    w.qn = s.take(M * D * e2);
    w.kn = s.take(M * D * e2);
    w.o1 = s.take(M * D * e2);
    w.lse1 = s.take((size_t)c.B * c.H * c.S * 4);
    w.a1 = s.take(M * D * e2);
    w.x1 = s.take(M * D * e2);
    w.n2 = s.take(M * D * e2);
    w.q2 = s.take(M * D * e2);
    w.kv2 = s.take(Mt * 2 * D * e2);
    w.q2n = s.take(M * D * e2);
    w.k2n = s.take(Mt * D * e2);
    w.o2 = s.take(M * D * e2);
    w.lse2 = s.take((size_t)c.B * c.H * c.S * 4);
    w.x2 = s.take(M * D * e2);
    w.n3 = s.take(M * D * e2);
    w.act = s.take(M * F * e2);
    w.pre = s.take(M * F * e2);
    w.f = s.take(M * D * e2);
    w.saved_total = s.off;
    Bump b;
    w.t_f2 = b.take(D * F * e2);
    w.t_f1 = b.take(D * F * e2);
    w.t_o2 = b.take(D * D * e2);
    w.t_q2 = b.take(D * D * e2);
    w.t_kv2 = b.take(2 * D * D * e2);
    w.t_o1 = b.take(D * D * e2);
    w.t_qkv1 = b.take(3 * D * D * e2);
    w.df = b.take(M * D * e2);
    w.dpre = b.take(M * F * e2);
    w.dn3 = b.take(M * D * e2);
    w.dx2 = b.take(M * D * e2);
    w.do2 = b.take(M * D * e2);
    w.dkv2 = b.take(Mt * 2 * D * e2);
    w.dq2n = b.take(M * D * e2);
    w.dk2n = b.take(Mt * D * e2);
    w.dq2 = b.take(M * D * e2);
    w.dn2 = b.take(M * D * e2);
    w.dx1 = b.take(M * D * e2);
    w.da1 = b.take(M * D * e2);
    w.do1 = b.take(M * D * e2);
    w.dqkv = b.take(M * 3 * D * e2);
    w.dqn = b.take(M * D * e2);
    w.dkn = b.take(M * D * e2);
    w.dn1 = b.take(M * D * e2);
    w.delta = b.take((size_t)c.B * c.H * c.S * 4);
    w.scratch_total = b.off;
    return w;
}

int check_cfg(const ftmi_wan_block_config& c) {
    if (c.B <= 0 || c.S <= 0 || c.T <= 0) return set_error(FTMI_ERR_INVALID, "wan_block: empty problem");
    if (c.H * 128 != c.D || c.D % 128 != 0 || c.D > 4096) return set_error(FTMI_ERR_UNSUPPORTED, "wan_block: width must be heads x 128, at most 4096");
    if (c.F <= 0 || (c.F % 64)) return set_error(FTMI_ERR_UNSUPPORTED, "wan_block: the feed-forward width must be a multiple of 64");
    return 0;
}

inline bf16_t* W(void* ws, size_t byte_off) { return reinterpret_cast<bf16_t*>(reinterpret_cast<char*>(ws) + byte_off); }
inline float* WF(void* ws, size_t byte_off) { return reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + byte_off); }

#define FTMI_TRY(x)          \
    do {                     \
        int _rc = (x);       \
        if (_rc) return _rc; \
    } while (0)

int linear(const bf16_t* X, long ldx, int M, int K, const bf16_t* Wm, const bf16_t* bias, int N, bf16_t* out, long ldo, int V, hipStream_t st) {
    GemmNtArgs a;
    a.X = X; a.ldx = ldx; a.W = Wm; a.ldw = K; a.M = M; a.N = N; a.K = K; a.bias = bias; a.out = out; a.ldo = ldo; a.variant = V;
    return gemm_nt(a, st);
}
// dW += dY^T X (fp32), db += column sums of dY
int linear_grads(const bf16_t* dy, long lddy, const bf16_t* inp, long ldi, int M, int N, int K, float* gw, float* gb, hipStream_t st) {
    GemmTnArgs t;
    t.U = dy; t.ldu = lddy; t.V = inp; t.ldv = ldi; t.C = gw; t.ldc = K; t.M = M; t.P = N; t.Q = K;
    FTMI_TRY(gemm_tn(t, st));
    WanRowArgs a;
    a.x = dy; a.ld_x = lddy; a.red1 = gb; a.rows = M; a.D = N; a.rows_per_batch = M;
    return wan_colsum(a, st);
}
WanRowArgs row_args(const bf16_t* x, long ldx, bf16_t* y, long ldy, int rows, int D, int rpb, float eps) {
    WanRowArgs a;
    a.x = x; a.ld_x = ldx; a.y = y; a.ld_y = ldy; a.rows = rows; a.D = D; a.rows_per_batch = rpb; a.eps = eps;
    return a;
}
AttnArgs attn_base(int B, int H, int Sq, int Sk) {
    AttnArgs a;
    a.B = B; a.H = H; a.Sq = Sq; a.Sk = Sk; a.d = 128;
    a.scale = 0.08838834764831845f;  // 1 / sqrt(128)
    return a;
}
inline void tok_strides(long& sb, long& sh, long& ss, long rows_per_batch, long ld) {
    sb = rows_per_batch * ld;
    sh = 128;
    ss = ld;
}

}  // namespace

size_t wan_block_saved_bytes(const ftmi_wan_block_config& c) { return make_layout(c).saved_total; }
size_t wan_block_scratch_bytes(const ftmi_wan_block_config& c) { return make_layout(c).scratch_total; }
size_t wan_block_param_elements(const ftmi_wan_block_config& c) { return offsets_of(c.D, c.F).total; }

int wan_block_forward(const ftmi_wan_block_config& c, const bf16_t* params, const bf16_t* x, const bf16_t* enc, const float* mod, const float* rope_cos,
                      const float* rope_sin, bf16_t* out, void* saved, size_t saved_bytes, hipStream_t st) {
    FTMI_TRY(check_cfg(c));
    const WanLayout L = make_layout(c);
    if (saved_bytes < L.saved_total) return set_error(FTMI_ERR_INVALID, "wan_block_forward: saved buffer too small");
    const Offsets O = offsets_of(c.D, c.F);
    const int B = c.B, S = c.S, T = c.T, D = c.D, F = c.F, M = B * S, Mt = B * T, V = c.gemm_variant;
    const float eps = c.eps;
    const long mb = 6L * D;  // sample stride of the modulation rows
    auto P = [&](size_t off) { return params + off; };
    auto MOD = [&](int i) { return mod + (size_t)i * D; };
    bf16_t *n1 = W(saved, L.n1), *qkv = W(saved, L.qkv), *qn = W(saved, L.qn), *kn = W(saved, L.kn), *o1 = W(saved, L.o1), *a1 = W(saved, L.a1), *x1 = W(saved, L.x1);
    // self-attention
    {
        WanRowArgs a = row_args(x, D, n1, D, M, D, S, eps);
        a.shift = MOD(0); a.scale = MOD(1); a.mod_bstride = mb;
        FTMI_TRY(wan_ln_fwd(a, st));
    }
    FTMI_TRY(linear(n1, D, M, D, P(O.w_qkv1), P(O.b_qkv1), 3 * D, qkv, 3 * D, V, st));
    for (int i = 0; i < 2; ++i) {
        WanRowArgs a = row_args(qkv + (size_t)i * D, 3 * D, i ? kn : qn, D, M, D, S, eps);
        a.w = P(i ? O.nk1 : O.nq1); a.rope_cos = rope_cos; a.rope_sin = rope_sin; a.head_dim = 128;
        FTMI_TRY(wan_rms_rope_fwd(a, st));
    }
    {
        AttnArgs a = attn_base(B, c.H, S, S);
        a.q = qn; tok_strides(a.q_sb, a.q_sh, a.q_ss, S, D);
        a.k = kn; tok_strides(a.k_sb, a.k_sh, a.k_ss, S, D);
        a.v = qkv + 2 * D; tok_strides(a.v_sb, a.v_sh, a.v_ss, S, 3 * D);
        a.o = o1; tok_strides(a.o_sb, a.o_sh, a.o_ss, S, D);
        a.lse2 = WF(saved, L.lse1);
        FTMI_TRY(attn_fwd(a, st));
    }
    FTMI_TRY(linear(o1, D, M, D, P(O.w_o1), P(O.b_o1), D, a1, D, V, st));
    {
        WanRowArgs a = row_args(x, D, x1, D, M, D, S, eps);
        a.scale = MOD(2); a.mod_bstride = mb; a.dy = a1; a.ld_dy = D;
        FTMI_TRY(wan_gate_res_fwd(a, st));
    }
    // cross-attention to the text tokens (no rotary embedding, no gate)
    bf16_t *n2 = W(saved, L.n2), *q2 = W(saved, L.q2), *kv2 = W(saved, L.kv2), *q2n = W(saved, L.q2n), *k2n = W(saved, L.k2n), *o2 = W(saved, L.o2), *x2 = W(saved, L.x2);
    {
        WanRowArgs a = row_args(x1, D, n2, D, M, D, S, eps);
        a.w = P(O.n2w); a.b = P(O.n2b);
        FTMI_TRY(wan_ln_fwd(a, st));
    }
    FTMI_TRY(linear(n2, D, M, D, P(O.w_q2), P(O.b_q2), D, q2, D, V, st));
    FTMI_TRY(linear(enc, D, Mt, D, P(O.w_kv2), P(O.b_kv2), 2 * D, kv2, 2 * D, V, st));
    {
        WanRowArgs a = row_args(q2, D, q2n, D, M, D, S, eps);
        a.w = P(O.nq2);
        FTMI_TRY(wan_rms_rope_fwd(a, st));
        WanRowArgs b = row_args(kv2, 2 * D, k2n, D, Mt, D, T, eps);
        b.w = P(O.nk2);
        FTMI_TRY(wan_rms_rope_fwd(b, st));
    }
    {
        AttnArgs a = attn_base(B, c.H, S, T);
        a.q = q2n; tok_strides(a.q_sb, a.q_sh, a.q_ss, S, D);
        a.k = k2n; tok_strides(a.k_sb, a.k_sh, a.k_ss, T, D);
        a.v = kv2 + D; tok_strides(a.v_sb, a.v_sh, a.v_ss, T, 2 * D);
        a.o = o2; tok_strides(a.o_sb, a.o_sh, a.o_ss, S, D);
        a.lse2 = WF(saved, L.lse2);
        FTMI_TRY(attn_fwd(a, st));
    }
    bf16_t* a2 = W(saved, L.f);  // (the feed-forward output buffer doubles as the staging of o2 W_o2^T + b: it is consumed by the next launch)
    FTMI_TRY(linear(o2, D, M, D, P(O.w_o2), P(O.b_o2), D, a2, D, V, st));
    {
        WanRowArgs a = row_args(x1, D, x2, D, M, D, S, eps);
        a.dy = a2; a.ld_dy = D;
        FTMI_TRY(wan_gate_res_fwd(a, st));
    }
    // feed-forward
    bf16_t *n3 = W(saved, L.n3), *act = W(saved, L.act), *pre = W(saved, L.pre), *f = W(saved, L.f);
    {
        WanRowArgs a = row_args(x2, D, n3, D, M, D, S, eps);
        a.shift = MOD(3); a.scale = MOD(4); a.mod_bstride = mb;
        FTMI_TRY(wan_ln_fwd(a, st));
    }
    {
        GemmNtArgs a;  // GELU-tanh, pre-activation kept
        a.X = n3; a.ldx = D; a.W = P(O.w_f1); a.ldw = D; a.M = M; a.N = F; a.K = D; a.bias = P(O.b_f1); a.out = act; a.ldo = F; a.out2 = pre; a.ldo2 = F;
        a.epi = EPI_GELU; a.variant = V;
        FTMI_TRY(gemm_nt(a, st));
    }
    FTMI_TRY(linear(act, F, M, F, P(O.w_f2), P(O.b_f2), D, f, D, V, st));
    {
        WanRowArgs a = row_args(x2, D, out, D, M, D, S, eps);
        a.scale = MOD(5); a.mod_bstride = mb; a.dy = f; a.ld_dy = D;
        FTMI_TRY(wan_gate_res_fwd(a, st));
    }
    return 0;
}

// grads: the block's flat fp32 gradient buffer (ADDED to); dmod fp32 [6, B, D] (ADDED to: column sums of d shift / d scale / d gate per sample);
// dx [B, S, D], denc [B, T, D] written.
int wan_block_backward(const ftmi_wan_block_config& c, const bf16_t* params, float* grads, const bf16_t* x, const bf16_t* enc, const float* mod,
                       const float* rope_cos, const float* rope_sin, const bf16_t* dout, bf16_t* dx, bf16_t* denc, float* dmod, void* saved,
                       size_t saved_bytes, void* scratch, size_t scratch_bytes, hipStream_t st) {
    FTMI_TRY(check_cfg(c));
    const WanLayout L = make_layout(c);
    if (saved_bytes < L.saved_total || scratch_bytes < L.scratch_total) return set_error(FTMI_ERR_INVALID, "wan_block_backward: buffer too small");
    const Offsets O = offsets_of(c.D, c.F);
    const int B = c.B, S = c.S, T = c.T, D = c.D, F = c.F, M = B * S, Mt = B * T, V = c.gemm_variant;
    const float eps = c.eps;
    const long mb = 6L * D;
    auto P = [&](size_t off) { return params + off; };
    auto G = [&](size_t off) { return grads + off; };
    auto MOD = [&](int i) { return mod + (size_t)i * D; };
    auto DMOD = [&](int i) { return dmod + (size_t)i * B * D; };
    // K-contiguous copies of the weights for the input-gradient GEMMs (dX = dY W as an NT GEMM against W^T)
    FTMI_TRY(transpose_bf16(P(O.w_f2), W(scratch, L.t_f2), D, F, st));
    FTMI_TRY(transpose_bf16(P(O.w_f1), W(scratch, L.t_f1), F, D, st));
    FTMI_TRY(transpose_bf16(P(O.w_o2), W(scratch, L.t_o2), D, D, st));
    FTMI_TRY(transpose_bf16(P(O.w_q2), W(scratch, L.t_q2), D, D, st));
    FTMI_TRY(transpose_bf16(P(O.w_kv2), W(scratch, L.t_kv2), 2 * D, D, st));
    FTMI_TRY(transpose_bf16(P(O.w_o1), W(scratch, L.t_o1), D, D, st));
    FTMI_TRY(transpose_bf16(P(O.w_qkv1), W(scratch, L.t_qkv1), 3 * D, D, st));
    const bf16_t *n1 = W(saved, L.n1), *qkv = W(saved, L.qkv), *qn = W(saved, L.qn), *kn = W(saved, L.kn), *o1 = W(saved, L.o1), *a1 = W(saved, L.a1), *x1 = W(saved, L.x1);
    const bf16_t *n2 = W(saved, L.n2), *q2 = W(saved, L.q2), *kv2 = W(saved, L.kv2), *q2n = W(saved, L.q2n), *k2n = W(saved, L.k2n), *o2 = W(saved, L.o2), *x2 = W(saved, L.x2);
    const bf16_t *n3 = W(saved, L.n3), *act = W(saved, L.act), *pre = W(saved, L.pre), *f = W(saved, L.f);

    // feed-forward branch: out = x2 + f * gate_ff
    bf16_t* df = W(scratch, L.df);
    {
        WanRowArgs a = row_args(dout, D, df, D, M, D, S, eps);
        a.scale = MOD(5); a.mod_bstride = mb; a.dy = f; a.ld_dy = D; a.red1 = DMOD(5); a.red_per_batch = 1;
        FTMI_TRY(wan_gate_res_bwd(a, st));
    }
    FTMI_TRY(linear_grads(df, D, act, F, M, D, F, G(O.w_f2), G(O.b_f2), st));
    bf16_t* dpre = W(scratch, L.dpre);
    {
        GemmNtArgs a;  // (d f W2) * gelu'(pre)
        a.X = df; a.ldx = D; a.W = W(scratch, L.t_f2); a.ldw = D; a.M = M; a.N = F; a.K = D; a.out = dpre; a.ldo = F; a.epi = EPI_DGELU; a.aux = pre; a.ldaux = F; a.variant = V;
        FTMI_TRY(gemm_nt(a, st));
    }
    FTMI_TRY(linear_grads(dpre, F, n3, D, M, F, D, G(O.w_f1), G(O.b_f1), st));
    bf16_t* dn3 = W(scratch, L.dn3);
    FTMI_TRY(linear(dpre, F, M, F, W(scratch, L.t_f1), nullptr, D, dn3, D, V, st));
    bf16_t* dx2 = W(scratch, L.dx2);
    {
        WanRowArgs a = row_args(x2, D, dx2, D, M, D, S, eps);
        a.scale = MOD(4); a.mod_bstride = mb; a.dy = dn3; a.ld_dy = D; a.dres = dout; a.red1 = DMOD(3); a.red2 = DMOD(4); a.red_per_batch = 1;
        FTMI_TRY(wan_ln_bwd(a, st));
    }
    // cross-attention branch: x2 = x1 + a2
    FTMI_TRY(linear_grads(dx2, D, o2, D, M, D, D, G(O.w_o2), G(O.b_o2), st));
    bf16_t* do2 = W(scratch, L.do2);
    FTMI_TRY(linear(dx2, D, M, D, W(scratch, L.t_o2), nullptr, D, do2, D, V, st));
    bf16_t *dkv2 = W(scratch, L.dkv2), *dq2n = W(scratch, L.dq2n), *dk2n = W(scratch, L.dk2n);
    {
        AttnArgs a = attn_base(B, c.H, S, T);
        a.q = q2n; tok_strides(a.q_sb, a.q_sh, a.q_ss, S, D);
        a.k = k2n; tok_strides(a.k_sb, a.k_sh, a.k_ss, T, D);
        a.v = kv2 + D; tok_strides(a.v_sb, a.v_sh, a.v_ss, T, 2 * D);
        a.o = const_cast<bf16_t*>(o2); tok_strides(a.o_sb, a.o_sh, a.o_ss, S, D);
        a.lse2 = WF(saved, L.lse2);
        a.dout = do2; tok_strides(a.do_sb, a.do_sh, a.do_ss, S, D);
        a.dq = dq2n; tok_strides(a.dq_sb, a.dq_sh, a.dq_ss, S, D);
        a.dk = dk2n; tok_strides(a.dk_sb, a.dk_sh, a.dk_ss, T, D);
        a.dv = dkv2 + D; tok_strides(a.dv_sb, a.dv_sh, a.dv_ss, T, 2 * D);
        a.delta = WF(scratch, L.delta);
        FTMI_TRY(attn_bwd(a, st));
    }
    bf16_t* dq2 = W(scratch, L.dq2);
    {
        WanRowArgs a = row_args(q2, D, dq2, D, M, D, S, eps);
        a.w = P(O.nq2); a.dy = dq2n; a.ld_dy = D; a.red2 = G(O.nq2);
        FTMI_TRY(wan_rms_rope_bwd(a, st));
        WanRowArgs b = row_args(kv2, 2 * D, dkv2, 2 * D, Mt, D, T, eps);
        b.w = P(O.nk2); b.dy = dk2n; b.ld_dy = D; b.red2 = G(O.nk2);
        FTMI_TRY(wan_rms_rope_bwd(b, st));
    }
    FTMI_TRY(linear_grads(dq2, D, n2, D, M, D, D, G(O.w_q2), G(O.b_q2), st));
    FTMI_TRY(linear_grads(dkv2, 2 * D, enc, D, Mt, 2 * D, D, G(O.w_kv2), G(O.b_kv2), st));
    FTMI_TRY(linear(dkv2, 2 * D, Mt, 2 * D, W(scratch, L.t_kv2), nullptr, D, denc, D, V, st));
    bf16_t* dn2 = W(scratch, L.dn2);
    FTMI_TRY(linear(dq2, D, M, D, W(scratch, L.t_q2), nullptr, D, dn2, D, V, st));
    bf16_t* dx1 = W(scratch, L.dx1);
    {
        WanRowArgs a = row_args(x1, D, dx1, D, M, D, S, eps);
        a.w = P(O.n2w); a.dy = dn2; a.ld_dy = D; a.dres = dx2; a.red1 = G(O.n2b); a.red2 = G(O.n2w);
        FTMI_TRY(wan_ln_bwd(a, st));
    }
    // self-attention branch: x1 = x + a1 * gate_msa
    bf16_t* da1 = W(scratch, L.da1);
    {
        WanRowArgs a = row_args(dx1, D, da1, D, M, D, S, eps);
        a.scale = MOD(2); a.mod_bstride = mb; a.dy = a1; a.ld_dy = D; a.red1 = DMOD(2); a.red_per_batch = 1;
        FTMI_TRY(wan_gate_res_bwd(a, st));
    }
    FTMI_TRY(linear_grads(da1, D, o1, D, M, D, D, G(O.w_o1), G(O.b_o1), st));
    bf16_t* do1 = W(scratch, L.do1);
    FTMI_TRY(linear(da1, D, M, D, W(scratch, L.t_o1), nullptr, D, do1, D, V, st));
    bf16_t *dqkv = W(scratch, L.dqkv), *dqn = W(scratch, L.dqn), *dkn = W(scratch, L.dkn);
    {
        AttnArgs a = attn_base(B, c.H, S, S);
        a.q = qn; tok_strides(a.q_sb, a.q_sh, a.q_ss, S, D);
        a.k = kn; tok_strides(a.k_sb, a.k_sh, a.k_ss, S, D);
        a.v = qkv + 2 * D; tok_strides(a.v_sb, a.v_sh, a.v_ss, S, 3 * D);
        a.o = const_cast<bf16_t*>(o1); tok_strides(a.o_sb, a.o_sh, a.o_ss, S, D);
        a.lse2 = WF(saved, L.lse1);
        a.dout = do1; tok_strides(a.do_sb, a.do_sh, a.do_ss, S, D);
        a.dq = dqn; tok_strides(a.dq_sb, a.dq_sh, a.dq_ss, S, D);
        a.dk = dkn; tok_strides(a.dk_sb, a.dk_sh, a.dk_ss, S, D);
        a.dv = dqkv + 2 * D; tok_strides(a.dv_sb, a.dv_sh, a.dv_ss, S, 3 * D);
        a.delta = WF(scratch, L.delta);
        FTMI_TRY(attn_bwd(a, st));
    }
    for (int i = 0; i < 2; ++i) {
        WanRowArgs a = row_args(qkv + (size_t)i * D, 3 * D, dqkv + (size_t)i * D, 3 * D, M, D, S, eps);
        a.w = P(i ? O.nk1 : O.nq1); a.dy = i ? dkn : dqn; a.ld_dy = D; a.red2 = G(i ? O.nk1 : O.nq1); a.rope_cos = rope_cos; a.rope_sin = rope_sin; a.head_dim = 128;
        FTMI_TRY(wan_rms_rope_bwd(a, st));
    }
    FTMI_TRY(linear_grads(dqkv, 3 * D, n1, D, M, 3 * D, D, G(O.w_qkv1), G(O.b_qkv1), st));
    bf16_t* dn1 = W(scratch, L.dn1);
    FTMI_TRY(linear(dqkv, 3 * D, M, 3 * D, W(scratch, L.t_qkv1), nullptr, D, dn1, D, V, st));  // the three projections' input gradients summed in the fp32 accumulator
    {
        WanRowArgs a = row_args(x, D, dx, D, M, D, S, eps);
        a.scale = MOD(1); a.mod_bstride = mb; a.dy = dn1; a.ld_dy = D; a.dres = dx1; a.red1 = DMOD(0); a.red2 = DMOD(1); a.red_per_batch = 1;
        FTMI_TRY(wan_ln_bwd(a, st));
    }
    return 0;
}


// ------------------------------------------------------------------------------------------------------------------------------------------------
// The same block for LoRA fine-tuning (the reference's Wan SFT recipes: --training_type lora, --target_modules "blocks.*(to_q|to_k|to_v|to_out.0)"):
// the base weights are FROZEN, fp32 adapters A [8, r, D] / B [8, D, r] sit on the eight attention projections, in the order
//   0 attn1.to_q, 1 attn1.to_k, 2 attn1.to_v, 3 attn1.to_out.0, 4 attn2.to_q, 5 attn2.to_k, 6 attn2.to_v, 7 attn2.to_out.0
// and every projection computes y = x W^T + b + s (x A^T) B^T, s = alpha / r, through the NT GEMM's K-extension (hy_dit.hip lora_linear_fwd; attn1's
// q|k|v stay ONE N = 3D launch with three adapters on one input and attn2's k|v ONE N = 2D launch over the text rows, laid out as ltx_dit.hip's fused QKV).
// The adapters are split into bf16 (hi, lo) planes once per call.  With r = 0 the launches are those of wan_block_forward, argument for argument.
//
// What the frozen base removes from the backward: the seven weight-gradient GEMMs, the bias / norm-weight / modulation / gate reductions (null
// reduction pointers), dmod, the seven weight transposes (K-contiguous twins arrive as pointers: the frozen base never invalidates them) and -- when
// denc == NULL, the text embedder being frozen too -- the [B T, 2D] x [2D, D] input-gradient GEMM into the text rows.
//
// saved (what the backward reads again):  n1, qkv, qn, kn, o1, lse1, x1, n2, q2, kv2, q2n, k2n, o2, lse2, x2, pre,
//                                         xa_qkv [M, 9r], xa_o1 [M, 3r], xa_q2 [M, 3r], xa_kv2 [Mt, 6r], xa_o2 [M, 3r]  (s x A^T as (hi | lo | hi) planes)
//   dropped against WanLayout: a1, n3, act, f -- read only by the gradients of frozen parameters (gate_msa, W_1, W_2, gate_ff): B S (3D + F) 2 bytes.
// scratch: forward transients (a1, n3, act, f, operand copies of A and B) overlaid with the backward's.
// Launcher calls per block (r > 0; an attention counts once): forward 2 splits + 5 down-projections + the full path's 19 = 26; backward 2 splits + 5
// down-projections + 10 adapter-gradient GEMMs + 18 of the full path's 39 (its 7 transposes, 7 weight-gradient GEMMs and 7 column sums are gone) = 35, 34
// without denc.
namespace {

struct WanLoraLayout {
    // saved
    size_t n1, qkv, qn, kn, o1, lse1, x1, n2, q2, kv2, q2n, k2n, o2, lse2, x2, pre, xa_qkv, xa_o1, xa_q2, xa_kv2, xa_o2, saved_total;
    // scratch, forward
    size_t a1, n3, act, f, a_sp, b_ext;
    // scratch, backward
    size_t df, dpre, dn3, dx2, do2, dkv2, dq2n, dk2n, dq2, dn2, dx1, da1, do1, dqkv, dqn, dkn, dn1, delta, dxa, bt_sp, at_ext, scratch_total;
};

WanLoraLayout make_lora_layout(const ftmi_wan_lora_block_config& c) {
    WanLoraLayout w;
    const size_t M = (size_t)c.B * c.S, Mt = (size_t)c.B * c.T, D = c.D, F = c.F, r = c.r > 0 ? c.r : 0, e2 = 2;
    Bump s;
    w.n1 = s.take(M * D * e2);
    w.qkv = s.take(M * 3 * D * e2);
    w.qn = s.take(M * D * e2);
    w.kn = s.take(M * D * e2);
    w.o1 = s.take(M * D * e2);
    w.lse1 = s.take((size_t)c.B * c.H * c.S * 4);
    w.x1 = s.take(M * D * e2);
    w.n2 = s.take(M * D * e2);
    w.q2 = s.take(M * D * e2);
    w.kv2 = s.take(Mt * 2 * D * e2);
    w.q2n = s.take(M * D * e2);
    w.k2n = s.take(Mt * D * e2);
    w.o2 = s.take(M * D * e2);
    w.lse2 = s.take((size_t)c.B * c.H * c.S * 4);
    w.x2 = s.take(M * D * e2);
    w.pre = s.take(M * F * e2);
    w.xa_qkv = s.take(M * 9 * r * e2);
    w.xa_o1 = s.take(M * 3 * r * e2);
    w.xa_q2 = s.take(M * 3 * r * e2);
    w.xa_kv2 = s.take(Mt * 6 * r * e2);
    w.xa_o2 = s.take(M * 3 * r * e2);
    w.saved_total = s.off;
    Bump f;  // forward and backward transients overlay each other
    w.a1 = f.take(M * D * e2);
    w.n3 = f.take(M * D * e2);
    w.act = f.take(M * F * e2);
    w.f = f.take(M * D * e2);
    w.a_sp = f.take(8 * 2 * r * D * e2);
    w.b_ext = f.take(8 * D * 3 * r * e2);
    Bump b;
    w.df = b.take(M * D * e2);
    w.dpre = b.take(M * F * e2);
    w.dn3 = b.take(M * D * e2);
    w.dx2 = b.take(M * D * e2);
    w.do2 = b.take(M * D * e2);
    w.dkv2 = b.take(Mt * 2 * D * e2);
    w.dq2n = b.take(M * D * e2);
    w.dk2n = b.take(Mt * D * e2);
    w.dq2 = b.take(M * D * e2);
    w.dn2 = b.take(M * D * e2);
    w.dx1 = b.take(M * D * e2);
    w.da1 = b.take(M * D * e2);
    w.do1 = b.take(M * D * e2);
    w.dqkv = b.take(M * 3 * D * e2);
    w.dqn = b.take(M * D * e2);
    w.dkn = b.take(M * D * e2);
    w.dn1 = b.take(M * D * e2);
    w.delta = b.take((size_t)c.B * c.H * c.S * 4);
    w.dxa = b.take((M > Mt ? M : Mt) * 9 * r * e2);
    w.bt_sp = b.take(8 * 2 * r * D * e2);
    w.at_ext = b.take(D * 24 * r * e2);
    w.scratch_total = f.off > b.off ? f.off : b.off;
    return w;
}

ftmi_wan_block_config base_cfg(const ftmi_wan_lora_block_config& c) {
    ftmi_wan_block_config b;
    b.B = c.B; b.S = c.S; b.T = c.T; b.D = c.D; b.H = c.H; b.F = c.F; b.eps = c.eps; b.gemm_variant = c.gemm_variant;
    return b;
}

int check_lora_cfg(const ftmi_wan_lora_block_config& c) {
    FTMI_TRY(check_cfg(base_cfg(c)));
    // (the split down-projection and the token-reduction GEMM work on whole groups of 64 adapter rows)
    if (c.r < 0 || (c.r % 64) != 0 || c.r > 128) return set_error(FTMI_ERR_UNSUPPORTED, "wan_lora_block: LoRA rank must be 0, 64 or 128 (pad other ranks with zeros)");
    if (c.r > 0 && c.D < 256) return set_error(FTMI_ERR_UNSUPPORTED, "wan_lora_block: adapters need a width of at least 256");
    return 0;
}

// the operand copies of one call's adapters and where its (hi | lo | hi) down-projections go
struct LoraOps {
    int r = 0;
    float s = 0.f;
    const bf16_t* sp = nullptr;   // forward: A as (hi, lo) row planes [8][2r][D];   backward: B^T planes [8][2r][D]
    const bf16_t* ext = nullptr;  // forward: B as [hi | hi | lo] columns [8][D][3r];   backward: A^T columns, the eight adapters side by side [D][24r]
};

// s * X A^T (or s * dY B) of `nadp` adjacent adapters as ONE split down-projection: out [rows, 3 nadp r]; X columns step by xk_stride per adapter (0: shared input)
int lora_down(const LoraOps& lo, const bf16_t* X, long ldx, int rows, int D, int adp, int nadp, long xk_stride, bf16_t* out, hipStream_t st) {
    const int r = lo.r;
    GemmNtArgs d;
    d.X = X; d.ldx = ldx; d.W = lo.sp + (size_t)adp * 2 * r * D; d.ldw = D; d.M = rows; d.N = 2 * nadp * r; d.K = D; d.alpha = lo.s; d.split_r = r;
    if (xk_stride > 0) { d.xk_grp_n = 2 * r; d.xk_grp_stride = xk_stride; }
    d.out = out; d.ldo = 3L * nadp * r; d.variant = 8;
    return gemm_nt(d, st);
}

// out [rows, nadp D] = X W^T + bias (+ the adapters adp .. adp + nadp - 1 on the same input X); xa [rows, 3 nadp r] is kept for the backward
int lora_linear_fwd(const LoraOps& lo, const bf16_t* X, int rows, int D, const bf16_t* Wm, const bf16_t* bias, int adp, int nadp, bf16_t* xa, bf16_t* out, int V,
                    hipStream_t st) {
    const int r = lo.r;
    GemmNtArgs a;
    a.X = X; a.ldx = D; a.W = Wm; a.ldw = D; a.M = rows; a.N = nadp * D; a.K = D; a.bias = bias; a.out = out; a.ldo = (long)nadp * D; a.variant = V;
    if (r > 0) {
        FTMI_TRY(lora_down(lo, X, D, rows, D, adp, nadp, 0, xa, st));
        a.X2 = xa; a.ldx2 = 3L * nadp * r; a.W2 = lo.ext + (size_t)adp * D * 3 * r; a.ldw2 = 3 * r; a.K2 = 3 * r;
        if (nadp > 1) { a.x2_grp_n = D; a.x2_grp_stride = 3 * r; }
    }
    return gemm_nt(a, st);
}

// dx [rows, D] = dY Wt^T (+ dXA A) (dx == nullptr: skipped), dB += dY^T XA, dA += dXA^T X for the adapters adp .. adp + nadp - 1 (dY [rows, nadp D])
int lora_linear_bwd(const LoraOps& lo, const bf16_t* X, const bf16_t* dy, int rows, int D, const bf16_t* Wt, int adp, int nadp, const bf16_t* xa, bf16_t* dxa,
                    bf16_t* dx, float* grad_a, float* grad_b, int V, hipStream_t st) {
    const int r = lo.r;
    const long lddy = (long)nadp * D;
    if (r > 0) FTMI_TRY(lora_down(lo, dy, lddy, rows, D, adp, nadp, nadp > 1 ? D : 0, dxa, st));
    if (dx) {
        GemmNtArgs a;
        a.X = dy; a.ldx = lddy; a.W = Wt; a.ldw = lddy; a.M = rows; a.N = D; a.K = nadp * D; a.out = dx; a.ldo = D; a.variant = V;
        if (r > 0) { a.X2 = dxa; a.ldx2 = 3L * nadp * r; a.W2 = lo.ext + (size_t)adp * 3 * r; a.ldw2 = 24L * r; a.K2 = 3 * nadp * r; }
        FTMI_TRY(gemm_nt(a, st));
    }
    if (r > 0) {
        GemmTnArgs t;  // dB += dY^T XA   (XA = hi + lo planes)
        t.U = dy; t.ldu = lddy; t.V = xa; t.ldv = 3L * nadp * r; t.v_fold = r; t.C = grad_b + (size_t)adp * D * r; t.ldc = r; t.M = rows; t.P = nadp * D; t.Q = r;
        if (nadp > 1) { t.v_grp_p = D; t.v_grp_stride = 3 * r; }
        FTMI_TRY(gemm_tn(t, st));
        GemmTnArgs u;  // dA += dXA^T X
        u.U = dxa; u.ldu = 3L * nadp * r; u.u_fold = r; u.V = X; u.ldv = D; u.C = grad_a + (size_t)adp * r * D; u.ldc = D; u.M = rows; u.P = nadp * r; u.Q = D;
        if (nadp > 1) { u.u_grp_p = r; u.u_grp_stride = 3 * r; }
        FTMI_TRY(gemm_tn(u, st));
    }
    return 0;
}

}  // namespace

size_t wan_lora_block_saved_bytes(const ftmi_wan_lora_block_config& c) { return make_lora_layout(c).saved_total; }
size_t wan_lora_block_scratch_bytes(const ftmi_wan_lora_block_config& c) { return make_lora_layout(c).scratch_total; }

// out == nullptr: the recomputation pass of gradient checkpointing -- the identical kernel sequence refills `saved` from the block's input and stops after
// the feed-forward's first GEMM (its pre-activation is the last thing the backward reads)
int wan_lora_block_forward(const ftmi_wan_lora_block_config& c, const ftmi_wan_lora_block_weights& w, const bf16_t* x, const bf16_t* enc, const float* mod,
                           const float* rope_cos, const float* rope_sin, bf16_t* out, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                           hipStream_t st) {
    FTMI_TRY(check_lora_cfg(c));
    const WanLoraLayout L = make_lora_layout(c);
    if (saved_bytes < L.saved_total || scratch_bytes < L.scratch_total) return set_error(FTMI_ERR_INVALID, "wan_lora_block_forward: buffer too small");
    if (c.r > 0 && (!w.lora_a || !w.lora_b)) return set_error(FTMI_ERR_INVALID, "wan_lora_block_forward: LoRA rank without adapters");
    const Offsets O = offsets_of(c.D, c.F);
    const bf16_t* params = reinterpret_cast<const bf16_t*>(w.params);
    const int B = c.B, S = c.S, T = c.T, D = c.D, F = c.F, M = B * S, Mt = B * T, V = c.gemm_variant, r = c.r;
    const float eps = c.eps;
    const long mb = 6L * D;
    auto P = [&](size_t off) { return params + off; };
    auto MOD = [&](int i) { return mod + (size_t)i * D; };
    LoraOps lo;
    lo.r = r; lo.s = c.lora_scale;
    if (r > 0) {  // operand copies of the fp32 adapters, once per call: A as (hi, lo) row planes, B as [hi | hi | lo] K-extension columns
        LoraSplitArgs sa;
        sa.w = w.lora_a; sa.rows = r; sa.cols = D; sa.nmat = 8; sa.in_bstride = (long)r * D; sa.sp = W(scratch, L.a_sp); sa.sp_bstride = 2L * r * D;
        FTMI_TRY(lora_split(sa, st));
        LoraSplitArgs sb;
        sb.w = w.lora_b; sb.rows = D; sb.cols = r; sb.nmat = 8; sb.in_bstride = (long)D * r; sb.ext = W(scratch, L.b_ext); sb.ext_bstride = 3L * D * r; sb.ld_ext = 3 * r;
        FTMI_TRY(lora_split(sb, st));
        lo.sp = W(scratch, L.a_sp); lo.ext = W(scratch, L.b_ext);
    }
    bf16_t *n1 = W(saved, L.n1), *qkv = W(saved, L.qkv), *qn = W(saved, L.qn), *kn = W(saved, L.kn), *o1 = W(saved, L.o1), *a1 = W(scratch, L.a1), *x1 = W(saved, L.x1);
    // self-attention
    {
        WanRowArgs a = row_args(x, D, n1, D, M, D, S, eps);
        a.shift = MOD(0); a.scale = MOD(1); a.mod_bstride = mb;
        FTMI_TRY(wan_ln_fwd(a, st));
    }
    FTMI_TRY(lora_linear_fwd(lo, n1, M, D, P(O.w_qkv1), P(O.b_qkv1), 0, 3, W(saved, L.xa_qkv), qkv, V, st));
    for (int i = 0; i < 2; ++i) {
        WanRowArgs a = row_args(qkv + (size_t)i * D, 3 * D, i ? kn : qn, D, M, D, S, eps);
        a.w = P(i ? O.nk1 : O.nq1); a.rope_cos = rope_cos; a.rope_sin = rope_sin; a.head_dim = 128;
        FTMI_TRY(wan_rms_rope_fwd(a, st));
    }
    {
        AttnArgs a = attn_base(B, c.H, S, S);
        a.q = qn; tok_strides(a.q_sb, a.q_sh, a.q_ss, S, D);
        a.k = kn; tok_strides(a.k_sb, a.k_sh, a.k_ss, S, D);
        a.v = qkv + 2 * D; tok_strides(a.v_sb, a.v_sh, a.v_ss, S, 3 * D);
        a.o = o1; tok_strides(a.o_sb, a.o_sh, a.o_ss, S, D);
        a.lse2 = WF(saved, L.lse1);
        FTMI_TRY(attn_fwd(a, st));
    }
    FTMI_TRY(lora_linear_fwd(lo, o1, M, D, P(O.w_o1), P(O.b_o1), 3, 1, W(saved, L.xa_o1), a1, V, st));
    {
        WanRowArgs a = row_args(x, D, x1, D, M, D, S, eps);
        a.scale = MOD(2); a.mod_bstride = mb; a.dy = a1; a.ld_dy = D;
        FTMI_TRY(wan_gate_res_fwd(a, st));
    }
    // cross-attention to the text tokens
    bf16_t *n2 = W(saved, L.n2), *q2 = W(saved, L.q2), *kv2 = W(saved, L.kv2), *q2n = W(saved, L.q2n), *k2n = W(saved, L.k2n), *o2 = W(saved, L.o2), *x2 = W(saved, L.x2);
    {
        WanRowArgs a = row_args(x1, D, n2, D, M, D, S, eps);
        a.w = P(O.n2w); a.b = P(O.n2b);
        FTMI_TRY(wan_ln_fwd(a, st));
    }
    FTMI_TRY(lora_linear_fwd(lo, n2, M, D, P(O.w_q2), P(O.b_q2), 4, 1, W(saved, L.xa_q2), q2, V, st));
    FTMI_TRY(lora_linear_fwd(lo, enc, Mt, D, P(O.w_kv2), P(O.b_kv2), 5, 2, W(saved, L.xa_kv2), kv2, V, st));
    {
        WanRowArgs a = row_args(q2, D, q2n, D, M, D, S, eps);
        a.w = P(O.nq2);
        FTMI_TRY(wan_rms_rope_fwd(a, st));
        WanRowArgs b = row_args(kv2, 2 * D, k2n, D, Mt, D, T, eps);
        b.w = P(O.nk2);
        FTMI_TRY(wan_rms_rope_fwd(b, st));
    }
    {
        AttnArgs a = attn_base(B, c.H, S, T);
        a.q = q2n; tok_strides(a.q_sb, a.q_sh, a.q_ss, S, D);
        a.k = k2n; tok_strides(a.k_sb, a.k_sh, a.k_ss, T, D);
        a.v = kv2 + D; tok_strides(a.v_sb, a.v_sh, a.v_ss, T, 2 * D);
        a.o = o2; tok_strides(a.o_sb, a.o_sh, a.o_ss, S, D);
        a.lse2 = WF(saved, L.lse2);
        FTMI_TRY(attn_fwd(a, st));
    }
    bf16_t* a2 = W(scratch, L.f);  // (the feed-forward output buffer doubles as the staging of o2 W_o2^T + b: it is consumed by the next launch)
    FTMI_TRY(lora_linear_fwd(lo, o2, M, D, P(O.w_o2), P(O.b_o2), 7, 1, W(saved, L.xa_o2), a2, V, st));
    {
        WanRowArgs a = row_args(x1, D, x2, D, M, D, S, eps);
        a.dy = a2; a.ld_dy = D;
        FTMI_TRY(wan_gate_res_fwd(a, st));
    }
    // feed-forward (frozen: only the pre-activation is kept)
    bf16_t *n3 = W(scratch, L.n3), *act = W(scratch, L.act), *pre = W(saved, L.pre), *f = W(scratch, L.f);
    {
        WanRowArgs a = row_args(x2, D, n3, D, M, D, S, eps);
        a.shift = MOD(3); a.scale = MOD(4); a.mod_bstride = mb;
        FTMI_TRY(wan_ln_fwd(a, st));
    }
    {
        GemmNtArgs a;  // GELU-tanh, pre-activation kept
        a.X = n3; a.ldx = D; a.W = P(O.w_f1); a.ldw = D; a.M = M; a.N = F; a.K = D; a.bias = P(O.b_f1); a.out = act; a.ldo = F; a.out2 = pre; a.ldo2 = F;
        a.epi = EPI_GELU; a.variant = V;
        FTMI_TRY(gemm_nt(a, st));
    }
    if (!out) return 0;
    FTMI_TRY(linear(act, F, M, F, P(O.w_f2), P(O.b_f2), D, f, D, V, st));
    {
        WanRowArgs a = row_args(x2, D, out, D, M, D, S, eps);
        a.scale = MOD(5); a.mod_bstride = mb; a.dy = f; a.ld_dy = D;
        FTMI_TRY(wan_gate_res_fwd(a, st));
    }
    return 0;
}

// dx [B, S, D] written; denc [B, T, D] written, or NULL (frozen text embedder: its GEMM is skipped); grad_a fp32 [8, r, D] / grad_b fp32 [8, D, r] ADDED to.
int wan_lora_block_backward(const ftmi_wan_lora_block_config& c, const ftmi_wan_lora_block_weights& w, const bf16_t* x, const bf16_t* enc, const float* mod,
                            const float* rope_cos, const float* rope_sin, const bf16_t* dout, bf16_t* dx, bf16_t* denc, float* grad_a, float* grad_b, void* saved,
                            size_t saved_bytes, void* scratch, size_t scratch_bytes, hipStream_t st) {
    FTMI_TRY(check_lora_cfg(c));
    const WanLoraLayout L = make_lora_layout(c);
    if (saved_bytes < L.saved_total || scratch_bytes < L.scratch_total) return set_error(FTMI_ERR_INVALID, "wan_lora_block_backward: buffer too small");
    if (c.r > 0 && (!w.lora_a || !w.lora_b || !grad_a || !grad_b)) return set_error(FTMI_ERR_INVALID, "wan_lora_block_backward: LoRA rank without adapters / gradient buffers");
    if (!w.w_qkv1_t || !w.w_o1_t || !w.w_q2_t || !w.w_kv2_t || !w.w_o2_t || !w.w_f1_t || !w.w_f2_t)
        return set_error(FTMI_ERR_INVALID, "wan_lora_block_backward: transposed weights missing");
    const Offsets O = offsets_of(c.D, c.F);
    const bf16_t* params = reinterpret_cast<const bf16_t*>(w.params);
    const int B = c.B, S = c.S, T = c.T, D = c.D, F = c.F, M = B * S, Mt = B * T, V = c.gemm_variant, r = c.r;
    const float eps = c.eps;
    const long mb = 6L * D;
    auto P = [&](size_t off) { return params + off; };
    auto MOD = [&](int i) { return mod + (size_t)i * D; };
    auto WT = [](const void* p) { return reinterpret_cast<const bf16_t*>(p); };
    LoraOps lo;
    lo.r = r; lo.s = c.lora_scale;
    if (r > 0) {
        LoraSplitArgs sb;  // B^T as (hi, lo) row planes: operand of dXA = s * dY B
        sb.w = w.lora_b; sb.rows = D; sb.cols = r; sb.nmat = 8; sb.in_bstride = (long)D * r; sb.t_sp = W(scratch, L.bt_sp); sb.t_sp_bstride = 2L * r * D;
        FTMI_TRY(lora_split(sb, st));
        LoraSplitArgs sa;  // A^T as K-extension columns, the eight adapters side by side [D, 24r]: dx += dXA A, fused projections take adjacent column groups
        sa.w = w.lora_a; sa.rows = r; sa.cols = D; sa.nmat = 8; sa.in_bstride = (long)r * D; sa.t_ext = W(scratch, L.at_ext); sa.t_ext_bstride = 3L * r; sa.ld_t_ext = 24L * r;
        FTMI_TRY(lora_split(sa, st));
        lo.sp = W(scratch, L.bt_sp); lo.ext = W(scratch, L.at_ext);
    }
    const bf16_t *n1 = W(saved, L.n1), *qkv = W(saved, L.qkv), *qn = W(saved, L.qn), *kn = W(saved, L.kn), *o1 = W(saved, L.o1), *x1 = W(saved, L.x1);
    const bf16_t *n2 = W(saved, L.n2), *q2 = W(saved, L.q2), *kv2 = W(saved, L.kv2), *q2n = W(saved, L.q2n), *k2n = W(saved, L.k2n), *o2 = W(saved, L.o2), *x2 = W(saved, L.x2);
    const bf16_t* pre = W(saved, L.pre);
    bf16_t* dxa = W(scratch, L.dxa);

    // feed-forward branch: out = x2 + f * gate_ff
    bf16_t* df = W(scratch, L.df);
    {
        WanRowArgs a = row_args(dout, D, df, D, M, D, S, eps);
        a.scale = MOD(5); a.mod_bstride = mb;
        FTMI_TRY(wan_gate_res_bwd(a, st));
    }
    bf16_t* dpre = W(scratch, L.dpre);
    {
        GemmNtArgs a;  // (d f W2) * gelu'(pre)
        a.X = df; a.ldx = D; a.W = WT(w.w_f2_t); a.ldw = D; a.M = M; a.N = F; a.K = D; a.out = dpre; a.ldo = F; a.epi = EPI_DGELU; a.aux = pre; a.ldaux = F; a.variant = V;
        FTMI_TRY(gemm_nt(a, st));
    }
    bf16_t* dn3 = W(scratch, L.dn3);
    FTMI_TRY(linear(dpre, F, M, F, WT(w.w_f1_t), nullptr, D, dn3, D, V, st));
    bf16_t* dx2 = W(scratch, L.dx2);
    {
        WanRowArgs a = row_args(x2, D, dx2, D, M, D, S, eps);
        a.scale = MOD(4); a.mod_bstride = mb; a.dy = dn3; a.ld_dy = D; a.dres = dout;
        FTMI_TRY(wan_ln_bwd(a, st));
    }
    // cross-attention branch: x2 = x1 + a2
    bf16_t* do2 = W(scratch, L.do2);
    FTMI_TRY(lora_linear_bwd(lo, o2, dx2, M, D, WT(w.w_o2_t), 7, 1, W(saved, L.xa_o2), dxa, do2, grad_a, grad_b, V, st));
    bf16_t *dkv2 = W(scratch, L.dkv2), *dq2n = W(scratch, L.dq2n), *dk2n = W(scratch, L.dk2n);
    {
        AttnArgs a = attn_base(B, c.H, S, T);
        a.q = q2n; tok_strides(a.q_sb, a.q_sh, a.q_ss, S, D);
        a.k = k2n; tok_strides(a.k_sb, a.k_sh, a.k_ss, T, D);
        a.v = kv2 + D; tok_strides(a.v_sb, a.v_sh, a.v_ss, T, 2 * D);
        a.o = const_cast<bf16_t*>(o2); tok_strides(a.o_sb, a.o_sh, a.o_ss, S, D);
        a.lse2 = WF(saved, L.lse2);
        a.dout = do2; tok_strides(a.do_sb, a.do_sh, a.do_ss, S, D);
        a.dq = dq2n; tok_strides(a.dq_sb, a.dq_sh, a.dq_ss, S, D);
        a.dk = dk2n; tok_strides(a.dk_sb, a.dk_sh, a.dk_ss, T, D);
        a.dv = dkv2 + D; tok_strides(a.dv_sb, a.dv_sh, a.dv_ss, T, 2 * D);
        a.delta = WF(scratch, L.delta);
        FTMI_TRY(attn_bwd(a, st));
    }
    bf16_t* dq2 = W(scratch, L.dq2);
    {
        WanRowArgs a = row_args(q2, D, dq2, D, M, D, S, eps);
        a.w = P(O.nq2); a.dy = dq2n; a.ld_dy = D;
        FTMI_TRY(wan_rms_rope_bwd(a, st));
        WanRowArgs b = row_args(kv2, 2 * D, dkv2, 2 * D, Mt, D, T, eps);
        b.w = P(O.nk2); b.dy = dk2n; b.ld_dy = D;
        FTMI_TRY(wan_rms_rope_bwd(b, st));
    }
    FTMI_TRY(lora_linear_bwd(lo, enc, dkv2, Mt, D, WT(w.w_kv2_t), 5, 2, W(saved, L.xa_kv2), dxa, denc, grad_a, grad_b, V, st));
    bf16_t* dn2 = W(scratch, L.dn2);
    FTMI_TRY(lora_linear_bwd(lo, n2, dq2, M, D, WT(w.w_q2_t), 4, 1, W(saved, L.xa_q2), dxa, dn2, grad_a, grad_b, V, st));
    bf16_t* dx1 = W(scratch, L.dx1);
    {
        WanRowArgs a = row_args(x1, D, dx1, D, M, D, S, eps);
        a.w = P(O.n2w); a.dy = dn2; a.ld_dy = D; a.dres = dx2;
        FTMI_TRY(wan_ln_bwd(a, st));
    }
    // self-attention branch: x1 = x + a1 * gate_msa
    bf16_t* da1 = W(scratch, L.da1);
    {
        WanRowArgs a = row_args(dx1, D, da1, D, M, D, S, eps);
        a.scale = MOD(2); a.mod_bstride = mb;
        FTMI_TRY(wan_gate_res_bwd(a, st));
    }
    bf16_t* do1 = W(scratch, L.do1);
    FTMI_TRY(lora_linear_bwd(lo, o1, da1, M, D, WT(w.w_o1_t), 3, 1, W(saved, L.xa_o1), dxa, do1, grad_a, grad_b, V, st));
    bf16_t *dqkv = W(scratch, L.dqkv), *dqn = W(scratch, L.dqn), *dkn = W(scratch, L.dkn);
    {
        AttnArgs a = attn_base(B, c.H, S, S);
        a.q = qn; tok_strides(a.q_sb, a.q_sh, a.q_ss, S, D);
        a.k = kn; tok_strides(a.k_sb, a.k_sh, a.k_ss, S, D);
        a.v = qkv + 2 * D; tok_strides(a.v_sb, a.v_sh, a.v_ss, S, 3 * D);
        a.o = const_cast<bf16_t*>(o1); tok_strides(a.o_sb, a.o_sh, a.o_ss, S, D);
        a.lse2 = WF(saved, L.lse1);
        a.dout = do1; tok_strides(a.do_sb, a.do_sh, a.do_ss, S, D);
        a.dq = dqn; tok_strides(a.dq_sb, a.dq_sh, a.dq_ss, S, D);
        a.dk = dkn; tok_strides(a.dk_sb, a.dk_sh, a.dk_ss, S, D);
        a.dv = dqkv + 2 * D; tok_strides(a.dv_sb, a.dv_sh, a.dv_ss, S, 3 * D);
        a.delta = WF(scratch, L.delta);
        FTMI_TRY(attn_bwd(a, st));
    }
    for (int i = 0; i < 2; ++i) {
        WanRowArgs a = row_args(qkv + (size_t)i * D, 3 * D, dqkv + (size_t)i * D, 3 * D, M, D, S, eps);
        a.w = P(i ? O.nk1 : O.nq1); a.dy = i ? dkn : dqn; a.ld_dy = D; a.rope_cos = rope_cos; a.rope_sin = rope_sin; a.head_dim = 128;
        FTMI_TRY(wan_rms_rope_bwd(a, st));
    }
    bf16_t* dn1 = W(scratch, L.dn1);  // the three projections' input gradients and their adapters' summed in the fp32 accumulator
    FTMI_TRY(lora_linear_bwd(lo, n1, dqkv, M, D, WT(w.w_qkv1_t), 0, 3, W(saved, L.xa_qkv), dxa, dn1, grad_a, grad_b, V, st));
    {
        WanRowArgs a = row_args(x, D, dx, D, M, D, S, eps);
        a.scale = MOD(1); a.mod_bstride = mb; a.dy = dn1; a.ld_dy = D; a.dres = dx1;
        FTMI_TRY(wan_ln_bwd(a, st));
    }
    return 0;
}

}  // namespace ftmi
