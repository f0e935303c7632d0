// CogVideoX DiT block stack, forward / backward orchestrator: one C call launches all L blocks (or a range of blocks of the backward) on the
// caller's stream; every activation the backward needs lives in the caller-provided workspace (no recompute), or -- cfg.checkpoint = 1, gradient
// checkpointing -- only the inputs of the blocks do, and the backward refills ONE block slot by running the block's forward launches again up to the
// feed-forward's pre-activation.  The same design as ltx_dit.hip, for the joint text+video block of CogVideoX (BASELINE config 3):
//
//   tokens [B, N = T + S, D] (text first)  ->  for each block:
//     n1 = LN(x) * (1 + scale) + shift            (CogVideoXLayerNormZero; text rows and video rows have their own shift / scale / gate)
//     q|k|v = n1 W_qkv^T + b  (+ LoRA, one fused GEMM with a grouped K-extension)    q, k <- per-head LayerNorm [+ RoPE on the video rows]
//     o = softmax(q k^T / 8) v   over all N joint tokens
//     h1 = x + gate * (o W_o^T + b + LoRA)
//     out = h1 + gate_ff * FF(LN(h1) * (1 + scale_ff) + shift_ff)                 (GELU-tanh, over text and video rows alike)
//
// Reference: [upstream] diffusers CogVideoXBlock as driven by finetrainers/models/cogvideox/base_specification.py:296-333, restated in
// oracle/cogvideox.py; the backward is the autograd backward of that graph with frozen base weights (dgrads only) and trainable LoRA A / B.
// The three projections q, k, v read the same n1: their input gradients are summed in one fp32 accumulator of the fused dgrad GEMM (the eager
// graph adds three bf16 tensors).
#include <string.h>

#include "common.hip.h"
#include "kernels.h"
#include "lora_proj.hip.h"

namespace ftmi {

namespace {

// What the forward walk reads of a workspace plan: the training layout (make_layout: one slot per block -- under gradient checkpointing one slot for
// all, blk_stride = 0 --, the inputs of blocks 1 .. L-1 kept) and the sampling layout (make_sample_plan: every block writes the SAME slot, blk_stride = 0,
// and the hidden state alternates between two buffers) share it.
struct CogFwdLayout {
    size_t mod_raw, tables, hs, blk0, blk_stride;
    int hs_slots = 1;                                         // block l > 0 reads slot (l - 1) % hs_slots of hs and block l < L - 1 writes slot l % hs_slots
    size_t n1, qkv, qn, kn, o, lse, xa_qkv, xa_o, h1, n2, z;  // per block, forward
    size_t s_act, s_f;
};
struct CogLayout : CogFwdLayout {
    size_t total = 0;
    size_t g_qkv, g_o, dxa_qkv, dxa_o;                        // per block, backward stash for the batched weight gradients
    size_t s_big, s_d1, s_d2, s_d3, s_dq, s_dk, s_dh0, s_dh1, s_delta;
};

// the forward entries of one block's slot, in the order both layouts keep them
void take_fwd_slot(CogFwdLayout& w, Bump& b, const ftmi_cog_config& c) {
    const size_t N = (size_t)c.T + c.S, M = (size_t)c.B * N, D = c.D, r = c.r > 0 ? c.r : 64, e2 = 2;
    w.n1 = b.take(M * D * e2);
    w.qkv = b.take(M * 3 * D * e2);
    w.qn = b.take(M * D * e2);
    w.kn = b.take(M * D * e2);
    w.o = b.take(M * D * e2);
    w.lse = b.take((size_t)c.B * c.H * N * 4);
    w.xa_qkv = b.take(M * 9 * r * e2);
    w.xa_o = b.take(M * 3 * r * e2);
    w.h1 = b.take(M * D * e2);
    w.n2 = b.take(M * D * e2);
    w.z = b.take(M * (size_t)c.D_ff * e2);
}

CogLayout make_layout(const ftmi_cog_config& c) {
    CogLayout w;
    const size_t N = (size_t)c.T + c.S, M = (size_t)c.B * N, D = c.D, r = c.r > 0 ? c.r : 64, e2 = 2;
    Bump g;
    w.mod_raw = g.take((size_t)c.B * c.L * 2 * 6 * D * e2);
    w.tables = g.take((size_t)c.L * 2 * 3 * c.B * 2 * D * e2);
    w.hs = g.take((size_t)(c.L > 1 ? c.L - 1 : 1) * M * D * e2);  // inputs of blocks 1 .. L-1
    w.hs_slots = c.L > 1 ? c.L - 1 : 1;
    Bump b;
    take_fwd_slot(w, b, c);
    w.g_qkv = b.take(M * 3 * D * e2);
    w.g_o = b.take(M * D * e2);
    w.dxa_qkv = b.take(M * 9 * r * e2);
    w.dxa_o = b.take(M * 3 * r * e2);
    // gradient checkpointing (cfg.checkpoint, the reference's --gradient_checkpointing: utils/activation_checkpoint.py:24-49 wraps every block): ONE block slot
    // that every block writes -- the forward leaves only hs behind, the backward refills the slot block by block (cog_block_forward, for_backward)
    w.blk_stride = c.checkpoint ? 0 : b.off;
    w.blk0 = g.take(b.off * (c.checkpoint ? 1 : c.L));
    w.s_act = g.take(M * (size_t)c.D_ff * e2);
    w.s_f = g.take(M * D * e2);
    w.s_big = g.take(M * (size_t)c.D_ff * e2);
    w.s_d1 = g.take(M * D * e2);
    w.s_d2 = g.take(M * D * e2);
    w.s_d3 = g.take(M * D * e2);
    w.s_dq = g.take(M * D * e2);
    w.s_dk = g.take(M * D * e2);
    w.s_dh0 = g.take(M * D * e2);
    w.s_dh1 = g.take(M * D * e2);
    w.s_delta = g.take((size_t)c.B * c.H * N * 4);
    w.total = g.off;
    return w;
}

int check_cfg(const ftmi_cog_config& c) {
    if (c.B <= 0 || c.S <= 0 || c.T < 0 || c.L <= 0) return set_error(FTMI_ERR_INVALID, "cog: empty problem");
    if (c.checkpoint != 0 && c.checkpoint != 1) return set_error(FTMI_ERR_INVALID, "cog: checkpoint must be 0 or 1");
    if (c.H * 64 != c.D || c.D % 128 != 0 || c.D > 4096) return set_error(FTMI_ERR_UNSUPPORTED, "cog: width must be heads x 64, a multiple of 128, at most 4096");
    if (c.r < 0 || (c.r % 64) != 0) return set_error(FTMI_ERR_UNSUPPORTED, "cog: LoRA rank must be 0 or a multiple of 64");
    if ((c.D_ff % 128) || (c.D_temb % 64)) return set_error(FTMI_ERR_UNSUPPORTED, "cog: D_ff must be a multiple of 128, the time-embedding width of 64");
    return 0;
}

struct Tables {  // the six modulation tables of one block, each [B][2][D]
    const bf16_t *shift1, *onep1, *gate1, *shift2, *onep2, *gate2;
};
Tables tables_of(const ftmi_cog_config& c, void* ws, const CogFwdLayout& L, int l) {
    const size_t one = (size_t)c.B * 2 * c.D;
    const bf16_t* t = W(ws, L.tables) + (size_t)l * 6 * one;
    return {t, t + one, t + 2 * one, t + 3 * one, t + 4 * one, t + 5 * one};
}

CogLnArgs ln_args(const ftmi_cog_config& c, const bf16_t* x, int which_norm, int l, const ftmi_cog_weights& w) {
    CogLnArgs a;
    a.x = x; a.rows = c.B * (c.T + c.S); a.D = c.D; a.rows_per_batch = c.T + c.S; a.seg0 = c.T; a.eps = c.eps_norm;
    a.w = P(w.norm_w, ((size_t)l * 2 + which_norm) * c.D);
    a.b = P(w.norm_b, ((size_t)l * 2 + which_norm) * c.D);
    return a;
}

int gate_res(const ftmi_cog_config& c, const bf16_t* res, const bf16_t* y, const bf16_t* gate, bf16_t* out, hipStream_t st) {
    CogLnArgs a;
    a.x = y; a.onep = gate; a.dres = res; a.y = out; a.rows = c.B * (c.T + c.S); a.D = c.D; a.rows_per_batch = c.T + c.S; a.seg0 = c.T;
    return cog_gate_residual(a, st);
}

AttnArgs attn_args(const ftmi_cog_config& c) {
    AttnArgs a;
    a.B = c.B; a.H = c.H; a.Sq = a.Sk = c.T + c.S; a.scale = 0.125f; a.d = 64;
    return a;
}
// q, k, o: token rows [B N, D]; v: the last D columns of the fused projection qkv [B N, 3D]
AttnArgs attn_args(const ftmi_cog_config& c, const bf16_t* q, const bf16_t* k, const bf16_t* qkv, bf16_t* o, float* lse) {
    AttnArgs a = attn_args(c);
    const long N = c.T + c.S, D = c.D;
    a.q = q; tok_strides(a.q_sb, a.q_sh, a.q_ss, N, D, 64);
    a.k = k; tok_strides(a.k_sb, a.k_sh, a.k_ss, N, D, 64);
    a.v = qkv + 2 * D; tok_strides(a.v_sb, a.v_sh, a.v_ss, N, 3 * D, 64);
    a.o = o; tok_strides(a.o_sb, a.o_sh, a.o_ss, N, D, 64);
    a.lse2 = lse;
    return a;
}

// One block's forward launches (the list at the top of this file): reads h0, fills the block's slot, writes the block's output to hout.
// for_backward: the recomputation pass of gradient checkpointing -- the same launches refill the slot and stop after the first feed-forward GEMM: its
// pre-activation z is the last thing the backward reads.  hout is then neither read nor written (for block L - 1 it would be the caller's tokens_out).
int cog_block_forward(const ftmi_cog_config& c, const ftmi_cog_weights& w, const CogFwdLayout& L, void* ws, int l, const bf16_t* h0, bf16_t* hout, bool for_backward,
                      hipStream_t st) {
    const int N = c.T + c.S, M = c.B * N, D = c.D, r = c.r, V = c.gemm_variant;
    const long D2 = (long)D * D;
    const float s = c.lora_scale;
    char* blk = reinterpret_cast<char*>(ws) + L.blk0 + L.blk_stride * l;
    const Tables t = tables_of(c, ws, L, l);
    const bf16_t* la = w.lora_a_sp ? P(w.lora_a_sp, (size_t)l * 4 * 2 * r * D) : nullptr;   // [4][2r][D]
    const bf16_t* lb = w.lora_b_ext ? P(w.lora_b_ext, (size_t)l * 4 * D * 3 * r) : nullptr;  // [4][D][3r]
    bf16_t* n1 = W(blk, L.n1);
    bf16_t* qkv = W(blk, L.qkv);

    {  // LayerNorm-zero 1
        CogLnArgs a = ln_args(c, h0, 0, l, w);
        a.shift = t.shift1; a.onep = t.onep1; a.y = n1;
        FTMI_TRY(cog_ln_mod_fwd(a, st));
    }
    {  // fused q|k|v projection (+ LoRA)
        GemmNtArgs a = linear_args(n1, D, M, P(w.w_qkv, (size_t)l * 3 * D2), D, 3 * D, D, P(w.b_qkv, (size_t)l * 3 * D), qkv, 3 * D, V);
        if (r > 0) {
            FTMI_TRY(gemm_nt(lora_down_args(n1, D, M, la, 3, D, r, s, W(blk, L.xa_qkv)), st));
            lora_ext_fwd(a, W(blk, L.xa_qkv), 3, r, lb);
        }
        FTMI_TRY(gemm_nt(a, st));
    }
    for (int qk = 0; qk < 2; ++qk) {  // per-head LayerNorm of q and k (+ RoPE on the video rows)
        CogLnArgs a;
        a.x = qkv + (size_t)qk * D; a.ld = 3 * D; a.y = W(blk, qk ? L.kn : L.qn); a.ld_out = D; a.rows = M; a.D = D; a.eps = c.eps_qk;
        a.w = P(w.qk_norm, ((size_t)l * 4 + qk * 2) * 64); a.b = P(w.qk_norm, ((size_t)l * 4 + qk * 2 + 1) * 64);
        a.cos = w.rope_cos; a.sin = w.rope_sin; a.rows_per_batch = N; a.seg0 = w.rope_cos ? c.T : 0;
        FTMI_TRY(cog_head_ln_fwd(a, st));
    }
    {  // joint attention
        FTMI_TRY(attn_fwd(attn_args(c, W(blk, L.qn), W(blk, L.kn), qkv, W(blk, L.o), WF(blk, L.lse)), st));
    }
    {  // to_out (+ LoRA), gated residual
        GemmNtArgs a = linear_args(W(blk, L.o), D, M, P(w.w_o, (size_t)l * D2), D, D, D, P(w.b_o, (size_t)l * D), W(ws, L.s_f), D, V);
        if (r > 0) {
            FTMI_TRY(gemm_nt(lora_down_args(W(blk, L.o), D, M, la + 3L * 2 * r * D, 1, D, r, s, W(blk, L.xa_o)), st));
            lora_ext_fwd(a, W(blk, L.xa_o), 1, r, lb + 3L * D * 3 * r);
        }
        FTMI_TRY(gemm_nt(a, st));
        FTMI_TRY(gate_res(c, h0, W(ws, L.s_f), t.gate1, W(blk, L.h1), st));
    }
    {  // LayerNorm-zero 2, feed-forward, gated residual
        CogLnArgs a = ln_args(c, W(blk, L.h1), 1, l, w);
        a.shift = t.shift2; a.onep = t.onep2; a.y = W(blk, L.n2);
        FTMI_TRY(cog_ln_mod_fwd(a, st));
        GemmNtArgs f1 = linear_args(W(blk, L.n2), D, M, P(w.w_ff1, (size_t)l * c.D_ff * D), D, c.D_ff, D, P(w.b_ff1, (size_t)l * c.D_ff), W(ws, L.s_act), c.D_ff, V);
        f1.out2 = W(blk, L.z); f1.ldo2 = c.D_ff; f1.epi = EPI_GELU;
        FTMI_TRY(gemm_nt(f1, st));
        if (for_backward) return 0;
        FTMI_TRY(gemm_nt(linear_args(W(ws, L.s_act), c.D_ff, M, P(w.w_ff2, (size_t)l * D * c.D_ff), c.D_ff, D, c.D_ff, P(w.b_ff2, (size_t)l * D), W(ws, L.s_f), D, V), st));
        FTMI_TRY(gate_res(c, W(blk, L.h1), W(ws, L.s_f), t.gate2, hout, st));
    }
    return 0;
}

// The forward walk over all L blocks, for either layout: the modulation GEMM + table pass, then per block the launches listed at the top of this file.
int cog_walk_forward(const ftmi_cog_config& c, const ftmi_cog_weights& w, const CogFwdLayout& L, const bf16_t* tokens_in, const bf16_t* temb_silu, bf16_t* tokens_out,
                     void* ws, hipStream_t st) {
    const int N = c.T + c.S, M = c.B * N, D = c.D, V = c.gemm_variant;

    // modulation of every LayerNorm-zero of every block: one GEMM over the stacked [L, 2, 6D, D_temb] weights, one table-building pass
    {
        const int nmod = c.L * 2 * 6 * D;
        FTMI_TRY(gemm_nt(linear_args(temb_silu, c.D_temb, c.B, P(w.mod_w, 0), c.D_temb, nmod, c.D_temb, P(w.mod_b, 0), W(ws, L.mod_raw), nmod, V), st));
        FTMI_TRY(cog_mod_tables(W(ws, L.mod_raw), W(ws, L.tables), c.L * 2, c.B, D, st));
    }

    for (int l = 0; l < c.L; ++l) {
        const bf16_t* h0 = l == 0 ? tokens_in : W(ws, L.hs) + (size_t)((l - 1) % L.hs_slots) * M * D;
        bf16_t* hout = l == c.L - 1 ? tokens_out : W(ws, L.hs) + (size_t)(l % L.hs_slots) * M * D;
        FTMI_TRY(cog_block_forward(c, w, L, ws, l, h0, hout, false, st));
    }
    return 0;
}

}  // namespace

size_t cog_workspace_bytes(const ftmi_cog_config& c) { return make_layout(c).total; }

int cog_blocks_forward(const ftmi_cog_config& c, const ftmi_cog_weights& w, const bf16_t* tokens_in, const bf16_t* temb_silu, bf16_t* tokens_out, void* ws,
                       size_t ws_bytes, hipStream_t st) {
    FTMI_TRY(check_cfg(c));
    const CogLayout L = make_layout(c);
    if (ws_bytes < L.total) return set_error(FTMI_ERR_INVALID, "cog_blocks_forward: workspace too small");
    return cog_walk_forward(c, w, L, tokens_in, temb_silu, tokens_out, ws, st);
}

// Blocks [l_lo, l_hi) of the backward, l_hi - 1 first.  d_out = gradient of block l_hi - 1's output when l_hi == L, otherwise the state left in the workspace by
// the previous call is continued.  When the call returns, grad_a / grad_b of its blocks are final (bucketed all-reduce); d_in (may be NULL) receives the gradient
// of block l_lo's input when l_lo == 0.
int cog_blocks_backward(const ftmi_cog_config& c, const ftmi_cog_weights& w, const bf16_t* tokens_in, const bf16_t* d_out, bf16_t* d_in, float* grad_a,
                        float* grad_b, void* ws, size_t ws_bytes, int l_hi, int l_lo, int accumulate, hipStream_t st) {
    FTMI_TRY(check_cfg(c));
    const CogLayout L = make_layout(c);
    if (ws_bytes < L.total) return set_error(FTMI_ERR_INVALID, "cog_blocks_backward: workspace too small");
    if (l_lo < 0 || l_hi > c.L || l_lo >= l_hi) return set_error(FTMI_ERR_INVALID, "cog_blocks_backward: bad block range");
    const int N = c.T + c.S, M = c.B * N, D = c.D, r = c.r, V = c.gemm_variant;
    const long D2 = (long)D * D;
    const float s = c.lora_scale;
    if (r > 0 && !accumulate) {  // the weight-gradient kernels accumulate: this range's slices start from zero
        const size_t off = (size_t)l_lo * 4 * r * D, nbytes = (size_t)(l_hi - l_lo) * 4 * r * D * sizeof(float);
        if (hipMemsetAsync(grad_a + off, 0, nbytes, st) != hipSuccess || hipMemsetAsync(grad_b + off, 0, nbytes, st) != hipSuccess)
            return set_error(FTMI_ERR_LAUNCH, "cog_blocks_backward: memset of the gradient buffer failed");
    }
    bf16_t* dh[2] = {W(ws, L.s_dh0), W(ws, L.s_dh1)};
    bf16_t *d1 = W(ws, L.s_d1), *d2 = W(ws, L.s_d2), *d3 = W(ws, L.s_d3);
    int cur = (c.L - l_hi) & 1;  // the gradient of the token stream ping-pongs between two buffers, one flip per finished block

    // LoRA weight gradients dB += dY^T XA, dA += dXA^T X of blocks [l0, l0 + nb): one batched launch per adapter group
    auto lora_wgrad = [&](int l0, int nb) -> int {
        char* blk0 = reinterpret_cast<char*>(ws) + L.blk0 + L.blk_stride * l0;
        const long bs = (long)(L.blk_stride / 2);
        struct G { size_t dy; long lddy; int nadp, adp; size_t xa, dxa, x; };
        const G groups[2] = {{L.g_o, D, 1, 3, L.xa_o, L.dxa_o, L.o}, {L.g_qkv, 3L * D, 3, 0, L.xa_qkv, L.dxa_qkv, L.n1}};
        float* ga = grad_a + (size_t)l0 * 4 * r * D;
        float* gb = grad_b + (size_t)l0 * 4 * D * r;
        for (const G& gr : groups) {
            GemmTnArgs tb = lora_db_args(W(blk0, gr.dy), gr.lddy, W(blk0, gr.xa), gr.nadp, r, D, gb + (size_t)gr.adp * D * r, M);  // dB[l] += dY[l]^T XA[l]
            tn_batch(tb, nb, bs, bs, 4L * D * r);
            FTMI_TRY(gemm_tn(tb, st));
            GemmTnArgs ta = lora_da_args(W(blk0, gr.dxa), gr.nadp, r, W(blk0, gr.x), D, D, ga + (size_t)gr.adp * r * D, M);  // dA[l] += dXA[l]^T X[l]
            tn_batch(ta, nb, bs, bs, 4L * r * D);
            FTMI_TRY(gemm_tn(ta, st));
        }
        return 0;
    };

    for (int l = l_hi - 1; l >= l_lo; --l) {
        char* blk = reinterpret_cast<char*>(ws) + L.blk0 + L.blk_stride * l;
        const bf16_t* h0 = l == 0 ? tokens_in : W(ws, L.hs) + (size_t)(l - 1) * M * D;
        const Tables t = tables_of(c, ws, L, l);
        const bf16_t* lat = w.lora_at_ext ? P(w.lora_at_ext, (size_t)l * 4 * D * 3 * r) : nullptr;  // [4][D][3r]
        const bf16_t* lbt = w.lora_bt_sp ? P(w.lora_bt_sp, (size_t)l * 4 * 2 * r * D) : nullptr;    // [4][2r][D]
        const bf16_t* dout = l == c.L - 1 ? d_out : dh[cur];
        bf16_t* dx = (l == 0 && d_in) ? d_in : dh[cur ^ 1];
        const bf16_t* qkv = W(blk, L.qkv);
        bf16_t* gqkv = W(blk, L.g_qkv);
        bf16_t* go = W(blk, L.g_o);
        if (c.checkpoint) FTMI_TRY(cog_block_forward(c, w, L, ws, l, h0, nullptr, true, st));  // the block's activations again, into the one slot

        // ---- feed-forward branch ----
        FTMI_TRY(gate_res(c, nullptr, dout, t.gate2, d1, st));  // d f = gate_ff * d out
        {
            GemmNtArgs a = linear_args(d1, D, M, P(w.w_ff2_t, (size_t)l * c.D_ff * D), D, c.D_ff, D, nullptr, W(ws, L.s_big), c.D_ff, V);
            a.epi = EPI_DGELU; a.aux = W(blk, L.z); a.ldaux = c.D_ff;
            FTMI_TRY(gemm_nt(a, st));
            FTMI_TRY(gemm_nt(linear_args(W(ws, L.s_big), c.D_ff, M, P(w.w_ff1_t, (size_t)l * D * c.D_ff), c.D_ff, D, c.D_ff, nullptr, d2, D, V), st));
            CogLnArgs n = ln_args(c, W(blk, L.h1), 1, l, w);
            n.onep = t.onep2; n.dy = d2; n.dres = dout; n.dx = d3;  // d3 = d h1
            FTMI_TRY(cog_ln_mod_bwd(n, st));
        }
        // ---- attention branch ----
        FTMI_TRY(gate_res(c, nullptr, d3, t.gate1, go, st));  // d(to_out output), kept for its weight gradient
        if (r > 0) FTMI_TRY(gemm_nt(lora_down_args(go, D, M, lbt + 3L * 2 * r * D, 1, D, r, s, W(blk, L.dxa_o)), st));
        {
            GemmNtArgs a = linear_args(go, D, M, P(w.w_o_t, (size_t)l * D2), D, D, D, nullptr, d1, D, V);
            if (r > 0) lora_ext_bwd(a, W(blk, L.dxa_o), 1, r, lat + 3L * D * 3 * r, 3 * r);
            FTMI_TRY(gemm_nt(a, st));  // d1 = d o
        }
        {
            AttnArgs a = attn_args(c, W(blk, L.qn), W(blk, L.kn), qkv, W(blk, L.o), WF(blk, L.lse));
            a.dout = d1;              tok_strides(a.do_sb, a.do_sh, a.do_ss, N, D, 64);
            a.delta = WF(ws, L.s_delta);
            a.dq = W(ws, L.s_dq);     tok_strides(a.dq_sb, a.dq_sh, a.dq_ss, N, D, 64);
            a.dk = W(ws, L.s_dk);     tok_strides(a.dk_sb, a.dk_sh, a.dk_ss, N, D, 64);
            a.dv = gqkv + 2 * D;      tok_strides(a.dv_sb, a.dv_sh, a.dv_ss, N, 3 * D, 64);
            FTMI_TRY(attn_bwd(a, st));
        }
        for (int qk = 0; qk < 2; ++qk) {  // head LayerNorm (+ RoPE) backward into the q / k thirds of d(q|k|v)
            CogLnArgs a;
            a.x = qkv + (size_t)qk * D; a.ld = 3 * D; a.dy = W(ws, qk ? L.s_dk : L.s_dq); a.ld_dy = D; a.dx = gqkv + (size_t)qk * D; a.ld_out = 3 * D;
            a.rows = M; a.D = D; a.eps = c.eps_qk; a.w = P(w.qk_norm, ((size_t)l * 4 + qk * 2) * 64);
            a.cos = w.rope_cos; a.sin = w.rope_sin; a.rows_per_batch = N; a.seg0 = w.rope_cos ? c.T : 0;
            FTMI_TRY(cog_head_ln_bwd(a, st));
        }
        if (r > 0) FTMI_TRY(gemm_nt(lora_down_args(gqkv, 3 * D, M, lbt, 3, D, r, s, W(blk, L.dxa_qkv), D), st));
        {
            GemmNtArgs a = linear_args(gqkv, 3 * D, M, P(w.w_qkv_t, (size_t)l * 3 * D2), 3 * D, D, 3 * D, nullptr, d2, D, V);  // d n1 = d(q|k|v) W_qkv + d XA A
            if (r > 0) lora_ext_bwd(a, W(blk, L.dxa_qkv), 3, r, P(w.lora_at_qkv_ext, (size_t)l * D * 9 * r), 9 * r);
            FTMI_TRY(gemm_nt(a, st));
            CogLnArgs n = ln_args(c, h0, 0, l, w);
            n.onep = t.onep1; n.dy = d2; n.dres = d3; n.dx = dx;
            FTMI_TRY(cog_ln_mod_bwd(n, st));
        }
        cur ^= 1;
        if (c.checkpoint && r > 0) FTMI_TRY(lora_wgrad(l, 1));  // the slot is about to be reused: this block's weight gradients now
    }
    if (r > 0 && !c.checkpoint) FTMI_TRY(lora_wgrad(l_lo, l_hi - l_lo));  // over the blocks of this range
    return 0;
}

// ---- latent sampling: the whole denoising loop of a validation run as ONE call (include/ftmi355.h: ftmi_cog_sample; the kernels are in sample_layout.hip) ----
// Restates what the reference gets from CogVideoXPipeline over the transformer it trains (finetrainers/models/cogvideox/base_specification.py:335-364), in
// latent space, text-to-video.  Before the loop the text projection fills the text rows of tokens_in [P B, T + S, D]; they are never written again.  Per step,
// on one stream, no host synchronisation -- the launches of MI355XCogVideoXTransformer3DModel.forward at batch P B, in its order, so the bits are its bits:
//   patch embedding                 one NT GEMM per model row over its S rows of cols, into the video rows of tokens_in
//   + sincos table (2b geometry)    cog_gate_residual per model row with a unit gate (text rows: + 0)
//   cog_walk_forward                the block walk over the sampling layout: every block writes the SAME slot, the hidden state alternates between two buffers
//   norm_final                      cog_ln_mod_fwd on the video rows of each model row (unit scale, zero shift)
//   norm_out                        cog_ln_mod_fwd with the step's shift / 1 + scale (one row for all: they share the timestep)
//   proj_out                        NT GEMM -> pred [P B S, Kc]
//   cog_sample_step                 guidance combine + DDIM update on the state, bf16 copies into cols
// Workspace: the modulation GEMM's output and tables (the only part that grows with L), tokens_in, the two hidden-state buffers, ONE block's forward slot, the
// two forward scratch buffers, nf / no of the head and pred.  None of the backward's stash or scratch areas.
// ftmi_cog_sample_ms is the same loop (cog_sample_loop, one body for both) whose last launch is cog_sample_step_dpm: the 5b / 1.5 checkpoints'
// CogVideoXDPMScheduler, which is what the reference's validation pipeline runs for them.  Its history, the previous step's x0 prediction, is one [B, S, Kc]
// fp32 buffer behind the DDIM workspace; the step's eight numbers (its guidance scale among them) and its noise slice come from device tables the caller filled.
namespace {

struct CogSamplePlan {
    CogFwdLayout lay;
    size_t tokens, nf, no, pred, total;
    long S, Kc;
    ftmi_cog_config bc;
};

int make_sample_plan(const ftmi_cog_sample_config& c, CogSamplePlan& p) {
    const ftmi_cog_sample_geometry& g = c.geo;
    if (g.B <= 0 || g.C <= 0 || g.F <= 0 || g.H <= 0 || g.W <= 0 || g.p <= 0 || g.pt <= 0 || c.T <= 0 || c.D_text <= 0 || c.steps <= 0)
        return set_error(FTMI_ERR_INVALID, "cog_sample: extents and steps must be positive");
    if (g.F % g.pt || g.H % g.p || g.W % g.p) return set_error(FTMI_ERR_UNSUPPORTED, "cog_sample: the latent size must be whole patches");
    if ((c.guidance != 1.0f) != (g.P == 2) || (g.P != 1 && g.P != 2)) return set_error(FTMI_ERR_INVALID, "cog_sample: P is 2 with guidance != 1 and 1 with guidance == 1");
    p.S = (long)(g.F / g.pt) * (g.H / g.p) * (g.W / g.p);
    p.Kc = (long)g.C * g.pt * g.p * g.p;
    if (p.Kc % 64 || p.Kc > 2048 || c.D_text % 64) return set_error(FTMI_ERR_UNSUPPORTED, "cog_sample: C pt p p and the text width must be multiples of 64 (GEMM)");
    if ((long)g.P * g.B * (c.T + p.S) > 0x7fffffffL) return set_error(FTMI_ERR_UNSUPPORTED, "cog_sample: too many tokens");
    ftmi_cog_config& b = p.bc;
    b.B = g.P * g.B; b.T = c.T; b.S = (int)p.S; b.D = c.D; b.H = c.heads; b.L = c.L; b.D_ff = c.D_ff; b.D_temb = c.D_temb; b.r = c.r;
    b.lora_scale = c.lora_scale; b.eps_norm = c.eps_norm; b.eps_qk = c.eps_qk; b.gemm_variant = c.gemm_variant;
    b.checkpoint = 0;  // no backward follows: the plan below is its own one-slot layout
    FTMI_TRY(check_cfg(b));
    const size_t M = (size_t)b.B * (c.T + p.S), Mv = (size_t)b.B * p.S, D = c.D, e2 = 2;
    Bump w;
    p.lay.mod_raw = w.take((size_t)b.B * c.L * 2 * 6 * D * e2);
    p.lay.tables = w.take((size_t)c.L * 2 * 3 * b.B * 2 * D * e2);
    p.tokens = w.take(M * D * e2);
    p.lay.hs = w.take(2 * M * D * e2);
    p.lay.hs_slots = 2;
    Bump slot;
    take_fwd_slot(p.lay, slot, b);
    p.lay.blk_stride = 0;
    p.lay.blk0 = w.take(slot.off);
    p.lay.s_act = w.take(M * (size_t)c.D_ff * e2);
    p.lay.s_f = w.take(M * D * e2);
    p.nf = w.take(Mv * D * e2);
    p.no = w.take(Mv * D * e2);
    p.pred = w.take(Mv * p.Kc * e2);
    p.total = w.off;
    return 0;
}

}  // namespace

size_t cog_sample_workspace_bytes(const ftmi_cog_sample_config& c) {
    CogSamplePlan p;
    return make_sample_plan(c, p) ? 0 : p.total;
}

namespace {

// The loop of both entry points.  step(i, pred): the launch that takes the step's prediction into the state and cols.  `need`: the entry point's workspace.
template <class Step>
int cog_sample_loop(const ftmi_cog_sample_config& c, const CogSamplePlan& p, size_t need, const ftmi_cog_sample_weights& w, bf16_t* cols, const bf16_t* text,
                    const bf16_t* temb_silu, const bf16_t* head_shift, const bf16_t* head_onep, void* ws, size_t ws_bytes, hipStream_t st, Step step) {
    if (ws_bytes < need) return set_error(FTMI_ERR_INVALID, "cog_sample: workspace too small (ftmi_cog_sample_workspace_bytes)");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return set_error(FTMI_ERR_INVALID, "cog_sample: the workspace must be 256-byte aligned");
    if (!w.patch_w || !w.patch_b || !w.text_w || !w.text_b || !w.norm_final_w || !w.norm_final_b || !w.norm_out_w || !w.norm_out_b || !w.proj_w || !w.proj_b ||
        !w.ones || !w.zeros || !w.blocks.mod_w || !w.blocks.w_qkv)
        return set_error(FTMI_ERR_INVALID, "cog_sample: weights missing");
    if (c.r > 0 && (!w.blocks.lora_a_sp || !w.blocks.lora_b_ext)) return set_error(FTMI_ERR_INVALID, "cog_sample: adapters of rank r without their working copies");
    if ((w.blocks.rope_cos != nullptr) != (w.blocks.rope_sin != nullptr)) return set_error(FTMI_ERR_INVALID, "cog_sample: the rotary tables come as a pair");
    if ((w.blocks.rope_cos != nullptr) == (w.pos != nullptr))
        return set_error(FTMI_ERR_INVALID, "cog_sample: a model has the sincos table (pos) or the rotary tables, one of the two");
    const ftmi_cog_sample_geometry& g = c.geo;
    const ftmi_cog_config& b = p.bc;
    const int D = c.D, T = c.T, S = (int)p.S, N = T + S, rows = b.B, Kc = (int)p.Kc, V = c.gemm_variant;
    bf16_t *tokens = W(ws, p.tokens), *nf = W(ws, p.nf), *no = W(ws, p.no), *pred = W(ws, p.pred);
    bf16_t* out = W(ws, p.lay.hs) + (size_t)((c.L - 1) % 2) * rows * N * D;  // the slot the last block would write if the walk went on: free while it runs

    for (int m = 0; m < rows; ++m)  // text rows, once: [neg; pos] through text_proj, one launch per model row as the model's forward issues them
        FTMI_TRY(gemm_nt(linear_args(text + (size_t)m * T * c.D_text, c.D_text, T, P(w.text_w, 0), c.D_text, D, c.D_text, P(w.text_b, 0), tokens + (size_t)m * N * D, D, V), st));

    for (int i = 0; i < c.steps; ++i) {
        for (int m = 0; m < rows; ++m) {
            bf16_t* tm = tokens + (size_t)m * N * D;
            FTMI_TRY(gemm_nt(linear_args(cols + (size_t)m * S * Kc, Kc, S, P(w.patch_w, 0), Kc, D, Kc, P(w.patch_b, 0), tm + (size_t)T * D, D, V), st));
            if (w.pos) {  // + sincos table (text rows: + 0), in place
                CogLnArgs a;
                a.x = tm; a.onep = P(w.ones, 0); a.dres = P(w.pos, 0); a.y = tm; a.rows = N; a.D = D; a.rows_per_batch = N; a.seg0 = 0;
                FTMI_TRY(cog_gate_residual(a, st));
            }
        }
        FTMI_TRY(cog_walk_forward(b, w.blocks, p.lay, tokens, temb_silu + (size_t)i * rows * c.D_temb, out, ws, st));
        for (int m = 0; m < rows; ++m) {  // norm_final on the video rows of a model row (contiguous; the model rows are T rows apart)
            CogLnArgs a;
            a.x = out + ((size_t)m * N + T) * D; a.w = P(w.norm_final_w, 0); a.b = P(w.norm_final_b, 0); a.shift = P(w.zeros, 0); a.onep = P(w.ones, 0);
            a.y = nf + (size_t)m * S * D; a.rows = S; a.D = D; a.rows_per_batch = S; a.seg0 = 0; a.eps = c.eps_norm;
            FTMI_TRY(cog_ln_mod_fwd(a, st));
        }
        {  // norm_out with the step's modulation (every model row shares the timestep: one table row), proj_out
            CogLnArgs a;
            a.x = nf; a.w = P(w.norm_out_w, 0); a.b = P(w.norm_out_b, 0); a.shift = head_shift + (size_t)i * D; a.onep = head_onep + (size_t)i * D;
            a.y = no; a.rows = rows * S; a.D = D; a.rows_per_batch = rows * S; a.seg0 = 0; a.eps = c.eps_norm;
            FTMI_TRY(cog_ln_mod_fwd(a, st));
            FTMI_TRY(gemm_nt(linear_args(no, D, rows * S, P(w.proj_w, 0), D, Kc, D, P(w.proj_b, 0), pred, Kc, V), st));
        }
        FTMI_TRY(step(i, pred));
    }
    return 0;
}

// The history of the multistep solver behind the DDIM plan: old fp32 [B, S, Kc] (p.total is a multiple of 256: the buffer is 16-byte aligned).
int make_sample_ms_plan(const ftmi_cog_sample_ms_config& c, CogSamplePlan& p, size_t& old_off, size_t& total) {
    if (c.solver != 1) return set_error(FTMI_ERR_UNSUPPORTED, "cog_sample_ms: solver 1 (DPM) is the one multistep solver");
    FTMI_TRY(make_sample_plan(c.base, p));
    Bump w;
    w.off = p.total;
    old_off = w.take((size_t)c.base.geo.B * p.S * p.Kc * sizeof(float));
    total = w.off;
    return 0;
}

}  // namespace

int cog_sample(const ftmi_cog_sample_config& c, const ftmi_cog_sample_weights& w, bf16_t* cols, float* x, const bf16_t* text, const bf16_t* temb_silu,
               const bf16_t* head_shift, const bf16_t* head_onep, const float* coef, void* ws, size_t ws_bytes, hipStream_t st) {
    CogSamplePlan p;
    FTMI_TRY(make_sample_plan(c, p));
    return cog_sample_loop(c, p, p.total, w, cols, text, temb_silu, head_shift, head_onep, ws, ws_bytes, st,
                           [&](int i, const bf16_t* pred) { return cog_sample_step(c.geo, pred, x, coef, i, c.guidance, cols, st); });
}

size_t cog_sample_ms_workspace_bytes(const ftmi_cog_sample_ms_config& c) {
    CogSamplePlan p;
    size_t old_off, total;
    return make_sample_ms_plan(c, p, old_off, total) ? 0 : total;
}

int cog_sample_ms(const ftmi_cog_sample_ms_config& c, const ftmi_cog_sample_weights& w, bf16_t* cols, float* x, const bf16_t* text, const bf16_t* temb_silu,
                  const bf16_t* head_shift, const bf16_t* head_onep, const float* coef, const float* noise, int noise_steps, void* ws, size_t ws_bytes,
                  hipStream_t st) {
    CogSamplePlan p;
    size_t old_off, total;
    FTMI_TRY(make_sample_ms_plan(c, p, old_off, total));
    // The rows live on the device; what the host knows is how many leading steps have a slice.  A step past them runs with no noise (its row has mn == 0).
    if (noise_steps < 0 || noise_steps > c.base.steps) return set_error(FTMI_ERR_INVALID, "cog_sample_ms: noise_steps counts the leading steps with a noise slice, 0 .. steps");
    if ((noise_steps > 0) != (noise != nullptr)) return set_error(FTMI_ERR_INVALID, "cog_sample_ms: noise goes with noise_steps > 0, and only with it");
    float* old = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + old_off);
    const size_t slice = (size_t)c.base.geo.B * p.S * p.Kc;
    return cog_sample_loop(c.base, p, total, w, cols, text, temb_silu, head_shift, head_onep, ws, ws_bytes, st, [&](int i, const bf16_t* pred) {
        return cog_sample_step_dpm(c.base.geo, pred, x, old, i < noise_steps ? noise + (size_t)i * slice : nullptr, coef + (size_t)i * 8, cols, st);
    });
}

}  // namespace ftmi
