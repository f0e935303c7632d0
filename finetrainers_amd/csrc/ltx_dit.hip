// LTX-Video DiT forward / backward orchestrator: one C call launches the whole 28-block forward (or
// backward) on the caller's stream -- O(1) host work per step instead of the reference's ~3-4k eager
// launches.  All activations the backward needs are stashed in the caller-provided workspace (about
// 0.4 GB per block at B=2, S=2688: trivial against 288 GB of HBM, so there is no activation recompute).
//
// Restates, op for op: finetrainers/patches/models/ltx_video/patch.py:38-127 (model-level forward) and
// the upstream LTXVideoTransformerBlock it iterates, with the peft LoRA branches of
// to_q/to_k/to_v/to_out.0 fused into the projections, and the autograd backward of the same graph with
// frozen base weights (dgrad only) and trainable LoRA A/B.
//
// Feed-forward adapters (the eight trailing pointers of ftmi_ltx_ff_weights, all NULL = none; peft attaches them when --target_modules names ff.net.0.proj and ff.net.2, as the default of
// trainer/control_trainer/config.py:60 does): two more adapters per block at the same rank, through the same builders (lora_proj.hip.h) and the block's
// proj_with / proj_bwd_with.  Their weight-gradient operands n2, g, dz and the gated dO are scratch shared by all blocks, so the backward writes n2 and g again
// per block (norm_modulate_fwd; gelu_from_pre on the kept z) and launches the four TN products inside the block loop -- see DESIGN.md 7-V.
#include <string.h>

#include "common.hip.h"
#include "kernels.h"
#include "lora_proj.hip.h"

namespace ftmi {

namespace {

struct WsLayout {
    size_t total = 0;
    size_t tsin, t1, emb, temb, ada, ada_out, cap_h, e, hs;
    // text-side K/V of the cross-attention for ALL blocks (the text stream `e` is block-independent): one launch each
    size_t kv2_all, k2n_all, xa_kv2_all, g_kv2_all, g_k2n_all, dxa_kv2_all;
    size_t blk0, blk_stride;
    // per-block (offsets relative to the block base)
    size_t n1, qkv, qrot, krot, o1, lse1, xa_qkv, xa_o, h1, q2raw, q2n, o2, lse2, xa_q2, xa_o2, h2, z;
    // per-block backward stash: the dY / dXA operands of the LoRA weight gradients, consumed by batched launches at the end
    size_t g_o2, g_q2, g_o, g_qkv, dxa_o2, dxa_q2, dxa_o, dxa_qkv;
    // scratch
    size_t s_n2, s_g, s_ln, s_dh0, s_dh1, s_d1, s_d2, s_d3, s_dqr, s_dkr, s_dbig, s_delta;
    size_t sk_flags;
    // feed-forward adapters (ff = true): their down-projected rows per block slot, the two dXA of the block in hand as scratch
    size_t xa_ff1 = 0, xa_ff2 = 0, s_dxa_ff1 = 0, s_dxa_ff2 = 0;
    size_t blk_slot;  // bytes of one block slot (blk_stride is 0 under gradient checkpointing: every block uses the same slot)
};

// A modulation group is a run of consecutive token rows that shares one timestep, i.e. one row of the conditioning tables: a whole sample in training and in
// text-to-video sampling ({B, S}), one latent frame of a sample where the timestep differs per frame ({B F, S / F}: ltx_forward_frames, ltx_sample_cond).
struct ModGroups { int n, rows; };
constexpr int kMaxModGroups = 128;  // 8 model rows (the batch cap of the sampler) x 16 latent frames (a 121-frame clip)

WsLayout make_layout(const ftmi_ltx_config& c, int groups = 0, bool ff = false) {
    WsLayout w;
    const size_t M = (size_t)c.B * c.S, Mt = (size_t)c.B * c.T, D = c.D, r = c.r > 0 ? c.r : 64;
    const size_t G = groups > 0 ? groups : c.B;  // rows of the conditioning tables
    const size_t e2 = 2;  // bf16
    Bump g;
    w.tsin = g.take(G * 256 * e2);
    w.t1 = g.take(G * D * e2);
    w.emb = g.take(G * D * e2);
    w.temb = g.take(G * 6 * D * e2);
    w.ada = g.take((size_t)c.L * G * 8 * D * e2);
    w.ada_out = g.take(G * 3 * D * e2);
    w.cap_h = g.take(Mt * D * e2);
    w.e = g.take(Mt * D * e2);
    w.hs = g.take((size_t)(c.L + 1) * M * D * e2);
    w.kv2_all = g.take(Mt * (size_t)c.L * 2 * D * e2);      // [Mt][L*2D]  (k | v per block)
    w.k2n_all = g.take(Mt * (size_t)c.L * D * e2);          // [Mt][L][D]
    w.xa_kv2_all = g.take(Mt * (size_t)c.L * 2 * 3 * r * e2);   // [Mt][L][k|v][hi|lo|hi][r]
    w.g_kv2_all = g.take(Mt * (size_t)c.L * 2 * D * e2);
    w.g_k2n_all = g.take(Mt * (size_t)c.L * D * e2);
    w.dxa_kv2_all = g.take(Mt * (size_t)c.L * 2 * 3 * r * e2);
    w.sk_flags = g.take(4096);  // 1024 int counters: one per 64-row tile of the token dimension (fused down-projection + GEMM launches, gemm_nt_lora_fused)
    Bump b;
    w.n1 = b.take(M * D * e2);
    w.qkv = b.take(M * 3 * D * e2);
    w.qrot = b.take(M * D * e2);
    w.krot = b.take(M * D * e2);
    w.o1 = b.take(M * D * e2);
    w.lse1 = b.take((size_t)c.B * c.H * c.S * 4);
    w.xa_qkv = b.take(M * 9 * r * e2);  // [M][q|k|v][hi|lo|hi][r]: fp32-equivalent s * x A^T as bf16 planes
    w.xa_o = b.take(M * 3 * r * e2);
    w.h1 = b.take(M * D * e2);
    w.q2raw = b.take(M * D * e2);
    w.q2n = b.take(M * D * e2);
    w.o2 = b.take(M * D * e2);
    w.lse2 = b.take((size_t)c.B * c.H * c.S * 4);
    w.xa_q2 = b.take(M * 3 * r * e2);
    w.xa_o2 = b.take(M * 3 * r * e2);
    w.h2 = b.take(M * D * e2);
    w.z = b.take(M * (size_t)c.D_ff * e2);
    w.g_o2 = b.take(M * D * e2);
    w.g_q2 = b.take(M * D * e2);
    w.g_o = b.take(M * D * e2);
    w.g_qkv = b.take(M * 3 * D * e2);
    w.dxa_o2 = b.take(M * 3 * r * e2);
    w.dxa_q2 = b.take(M * 3 * r * e2);
    w.dxa_o = b.take(M * 3 * r * e2);
    w.dxa_qkv = b.take(M * 9 * r * e2);
    if (ff) {  // (after everything the eight-adapter slot holds: that layout is a prefix of this one)
        w.xa_ff1 = b.take(M * 3 * r * e2);
        w.xa_ff2 = b.take(M * 3 * r * e2);
    }
    // gradient checkpointing (cfg.checkpoint, the reference's --gradient_checkpointing: utils/activation_checkpoint.py:24-49 wraps every block): ONE block slot
    // instead of L -- a block keeps only its input (the residual stream hs[l], kept for every block either way) and its forward runs again inside its backward
    w.blk_slot = b.off;
    w.blk_stride = c.checkpoint ? 0 : b.off;
    w.blk0 = g.take(w.blk_slot * (c.checkpoint ? 1 : c.L));
    w.s_n2 = g.take(M * D * e2);
    w.s_g = g.take(M * (size_t)c.D_ff * e2);
    w.s_ln = g.take(M * D * e2);
    w.s_dh0 = g.take(M * D * e2);
    w.s_dh1 = g.take(M * D * e2);
    w.s_d1 = g.take(M * D * e2);
    w.s_d2 = g.take(M * D * e2);
    w.s_d3 = g.take(M * D * e2);
    w.s_dqr = g.take(M * D * e2);
    w.s_dkr = g.take(M * D * e2);
    w.s_dbig = g.take(M * (size_t)c.D_ff * e2);
    w.s_delta = g.take((size_t)c.B * c.H * c.S * 4);
    if (ff) {
        w.s_dxa_ff1 = g.take(M * 3 * r * e2);
        w.s_dxa_ff2 = g.take(M * 3 * r * e2);
    }
    w.total = g.off;
    return w;
}

// frames > 0: the per-frame entries, whose timestep embedding runs in chunks of 8 rows -- the bound is on the modulation groups B x frames, not on B
int check_cfg(const ftmi_ltx_config& c, int frames = 0) {
    if (c.B <= 0 || c.S <= 0 || c.T <= 0 || c.L <= 0) return set_error(FTMI_ERR_INVALID, "ltx: empty problem");
    if (c.D != 2048 || c.H * 64 != c.D) return set_error(FTMI_ERR_UNSUPPORTED, "ltx: kernels are built for width 2048 = 32 heads x 64");
    if (frames <= 0 && c.B > 8) return set_error(FTMI_ERR_UNSUPPORTED, "ltx: per-rank batch must be <= 8 (timestep-embedding kernel)");
    if (frames > 0 && (c.S % frames != 0 || (long)c.B * frames > kMaxModGroups))
        return set_error(FTMI_ERR_UNSUPPORTED, "ltx: per-frame timesteps need S % frames == 0 and batch x frames <= 128 (8 model rows x 16 latent frames)");
    if (c.r < 0 || (c.r % 64) != 0) return set_error(FTMI_ERR_UNSUPPORTED, "ltx: LoRA rank must be 0 or a multiple of 64");
    if ((c.C_in % 64) || (c.C_out % 64) || (c.D_ff % 128) || (c.D_cap % 64))
        return set_error(FTMI_ERR_UNSUPPORTED, "ltx: channel counts must be multiples of 64");
    if (c.d_valid < 0 || c.d_valid > c.D || c.head_dim_valid < 0 || c.head_dim_valid > 64)
        return set_error(FTMI_ERR_INVALID, "ltx: d_valid / head_dim_valid describe a model narrower than the layout (0 = full width)");
    return 0;
}

// The feed-forward adapters of a call (the extension of ftmi_ltx_ff_weights): typed operand copies, `on` = all eight present.  All eight null: none.
struct FfOps {
    bool on = false;
    const bf16_t *a1_sp = nullptr, *a1t_ext = nullptr, *b1_ext = nullptr, *b1t_sp = nullptr, *a2_sp = nullptr, *a2t_ext = nullptr, *b2_ext = nullptr, *b2t_sp = nullptr;
};
int ff_ops(const ftmi_ltx_config& c, const ftmi_ltx_ff_weights& w, FfOps* o) {
    *o = FfOps();
    const void* p[8] = {w.ff_a1_sp, w.ff_a1t_ext, w.ff_b1_ext, w.ff_b1t_sp, w.ff_a2_sp, w.ff_a2t_ext, w.ff_b2_ext, w.ff_b2t_sp};
    int n = 0;
    for (const void* q : p) n += q != nullptr;
    if (n == 0) return 0;
    if (n != 8) return set_error(FTMI_ERR_INVALID, "ltx: feed-forward adapters need all eight operand copies (or none)");
    if (c.r <= 0) return set_error(FTMI_ERR_INVALID, "ltx: feed-forward adapters take the model's rank, which is 0");
    o->on = true;
    o->a1_sp = P(p[0], 0); o->a1t_ext = P(p[1], 0); o->b1_ext = P(p[2], 0); o->b1t_sp = P(p[3], 0);
    o->a2_sp = P(p[4], 0); o->a2t_ext = P(p[5], 0); o->b2_ext = P(p[6], 0); o->b2t_sp = P(p[7], 0);
    return 0;
}

// A projection with its LoRA: the down-projection `dn` (writes a.X2) and the GEMM `a` (K-extension over X2) -- one fused launch where the pair is eligible
// (gemm_nt_lora_fused: FTMI_FUSE_DOWN=1), else the two launches of rounds 1-5.  `fx` = the workspace's row-tile counters + the running expectation of this call.
struct FuseCtx { int* flags; int expect; };
int lora_gemm(const GemmNtArgs& a, const GemmNtArgs& dn, FuseCtx& fx, hipStream_t st) {
    return gemm_nt_lora_fused(a, dn, (a.M + 63) / 64 <= 1024 ? fx.flags : nullptr, &fx.expect, st);
}

AttnArgs attn_args(const ftmi_ltx_config& c, int Sq, int Sk) {
    AttnArgs a;
    a.B = c.B; a.H = c.H; a.Sq = Sq; a.Sk = Sk;
    a.scale = (c.head_dim_valid > 0 && c.head_dim_valid < 64) ? 1.0f / sqrtf((float)c.head_dim_valid) : 0.125f;  // (a zero-padded narrow head: the scale of its true width)
    return a;
}
// self-attention over a block slot: q, k, o token rows [B S, D]; v the last D columns of the fused projection qkv [B S, 3D]
AttnArgs self_attn_args(const ftmi_ltx_config& c, const WsLayout& L, char* blk) {
    const long D = c.D;
    AttnArgs a = attn_args(c, c.S, c.S);
    a.q = W(blk, L.qrot); tok_strides(a.q_sb, a.q_sh, a.q_ss, c.S, D, 64);
    a.k = W(blk, L.krot); tok_strides(a.k_sb, a.k_sh, a.k_ss, c.S, D, 64);
    a.v = W(blk, L.qkv) + 2 * D; tok_strides(a.v_sb, a.v_sh, a.v_ss, c.S, 3 * D, 64);
    a.o = W(blk, L.o1); tok_strides(a.o_sb, a.o_sh, a.o_ss, c.S, D, 64);
    a.lse2 = WF(blk, L.lse1);
    return a;
}
// cross-attention of block l with the text-mask bias: its keys / values are block l's columns of the all-block arrays [B T, L D] / [B T, L 2D]
AttnArgs cross_attn_args(const ftmi_ltx_config& c, const WsLayout& L, void* ws, char* blk, int l, const float* key_bias) {
    const long D = c.D;
    AttnArgs a = attn_args(c, c.S, c.T);
    a.q = W(blk, L.q2n); tok_strides(a.q_sb, a.q_sh, a.q_ss, c.S, D, 64);
    a.k = W(ws, L.k2n_all) + (size_t)l * D; tok_strides(a.k_sb, a.k_sh, a.k_ss, c.T, c.L * D, 64);
    a.v = W(ws, L.kv2_all) + (size_t)l * 2 * D + D; tok_strides(a.v_sb, a.v_sh, a.v_ss, c.T, c.L * 2 * D, 64);
    a.o = W(blk, L.o2); tok_strides(a.o_sb, a.o_sh, a.o_ss, c.S, D, 64);
    a.lse2 = WF(blk, L.lse2); a.kbias = key_bias; a.kb_sb = c.T;
    return a;
}

}  // namespace

// (the planners return a size: a combination ff_ops refuses plans nothing)
size_t ltx_workspace_bytes(const ftmi_ltx_config& c, const ftmi_ltx_ff_weights& w) {
    FfOps ff;
    return ff_ops(c, w, &ff) == 0 ? make_layout(c, 0, ff.on).total : 0;
}

int ltx_workspace_offset(const ftmi_ltx_config& c, const ftmi_ltx_ff_weights& w, const char* name, int layer, size_t* off) {
    FfOps fo;
    FTMI_TRY(ff_ops(c, w, &fo));
    const WsLayout L = make_layout(c, 0, fo.on);
    const size_t M = (size_t)c.B * c.S;
    struct E { const char* n; size_t o; };
    const E globals[] = {{"kv2_all", L.kv2_all}, {"k2n_all", L.k2n_all}, {"xa_kv2_all", L.xa_kv2_all}, {"e", L.e}, {"emb", L.emb}, {"temb", L.temb}, {"ada", L.ada}, {"ada_out", L.ada_out}, {"tsin", L.tsin}};
    for (const E& g : globals)
        if (!strcmp(name, g.n)) { *off = g.o; return 0; }
    if (!strcmp(name, "hs")) {
        if (layer < 0 || layer > c.L) return set_error(FTMI_ERR_INVALID, "workspace_offset: layer out of range");
        *off = L.hs + (size_t)layer * M * c.D * 2;
        return 0;
    }
    const E blocks[] = {{"n1", L.n1}, {"qkv", L.qkv}, {"qrot", L.qrot}, {"krot", L.krot}, {"o1", L.o1}, {"lse1", L.lse1},
                        {"xa_qkv", L.xa_qkv}, {"xa_o", L.xa_o}, {"h1", L.h1}, {"q2raw", L.q2raw}, {"q2n", L.q2n},
                        {"o2", L.o2}, {"lse2", L.lse2}, {"xa_q2", L.xa_q2},
                        {"xa_o2", L.xa_o2}, {"h2", L.h2}, {"z", L.z}};
    if (layer < 0 || layer >= c.L) return set_error(FTMI_ERR_INVALID, "workspace_offset: layer out of range");
    for (const E& b : blocks)
        if (!strcmp(name, b.n)) { *off = L.blk0 + L.blk_stride * layer + b.o; return 0; }
    if (fo.on) {
        const E ffb[] = {{"xa_ff1", L.xa_ff1}, {"xa_ff2", L.xa_ff2}};
        for (const E& b : ffb)
            if (!strcmp(name, b.n)) { *off = L.blk0 + L.blk_stride * layer + b.o; return 0; }
    }
    return set_error(FTMI_ERR_INVALID, "workspace_offset: unknown name");
}

// One transformer block of the forward (steps 1-13 of patches/models/ltx_video/patch.py:82-123 + the upstream block): reads hs[l], writes hs[l+1] and the
// block's activations into its slot.  Called by the forward for every block and -- under gradient checkpointing -- again by the backward right before a
// block's gradient computation (deterministic kernels: the recomputed activations are the forward's, bit for bit).
static int ltx_block_forward(const ftmi_ltx_config& c, const ftmi_ltx_weights& w, const FfOps& ff, const WsLayout& L, void* ws, int l, const float* key_bias, hipStream_t st,
                             FuseCtx& fx, const ModGroups& mg) {
    const int M = c.B * c.S, D = c.D, r = c.r, V = c.gemm_variant;
    const long D2 = (long)D * D;
    const float s = c.lora_scale;
    {
        char* blk = reinterpret_cast<char*>(ws) + L.blk0 + L.blk_stride * l;
        const bf16_t* h0 = W(ws, L.hs) + (size_t)l * M * D;
        bf16_t* hout = W(ws, L.hs) + (size_t)(l + 1) * M * D;
        const bf16_t* ada = W(ws, L.ada) + (size_t)l * mg.n * 8 * D;  // [groups][8][D]: one row per sample, or per latent frame of a sample
        const long ab = 8L * D;
        const bf16_t* la = w.lora_a_sp ? P(w.lora_a_sp, (size_t)l * 8 * 2 * r * D) : nullptr;   // [8][2r][D]  (hi, lo) planes of A
        const bf16_t* lb = w.lora_b_ext ? P(w.lora_b_ext, (size_t)l * 8 * D * 3 * r) : nullptr;  // [8][D][3r]  [B_hi | B_hi | B_lo]
        bf16_t* n1 = W(blk, L.n1);
        bf16_t* qkv = W(blk, L.qkv);
        // the projection `a` (+ the adapters adp .. adp + nadp - 1 on its input, xa [M, 3 nadp r] kept for the backward)
        // the same for any operand pair: sp = the (hi, lo) row planes of A [nadp 2r, a.K], b_ext [a.N, 3r] (the feed-forward adapters are rectangular)
        auto proj_with = [&](GemmNtArgs& a, const bf16_t* sp, const bf16_t* b_ext, int nadp, bf16_t* xa) -> int {
            lora_ext_fwd(a, xa, nadp, r, b_ext);
            return lora_gemm(a, lora_down_args(a.X, a.ldx, M, sp, nadp, a.K, r, s, xa), fx, st);
        };
        auto proj = [&](GemmNtArgs& a, int adp, int nadp, bf16_t* xa) -> int {
            if (r <= 0) return gemm_nt(a, st);
            return proj_with(a, la + (size_t)adp * 2 * r * D, lb + (size_t)adp * D * 3 * r, nadp, xa);
        };

        // 1. norm1 + AdaLN modulate
        FTMI_TRY(norm_modulate_fwd(h0, ada + 0 * D, ada + 6 * D, ab, n1, M, mg.rows, D, c.eps_norm, 0, st));
        // 2-3. fused q,k,v projection (+ LoRA)
        {
            GemmNtArgs a = linear_args(n1, D, M, P(w.w_qkv, (size_t)l * 3 * D2), D, 3 * D, D, P(w.b_qkv, (size_t)l * 3 * D), qkv, 3 * D, V);
            FTMI_TRY(proj(a, 0, 3, W(blk, L.xa_qkv)));
        }
        // 4. QK RMSNorm across heads + RoPE
        FTMI_TRY(qknorm_rope_fwd(qkv, 3 * D, P(w.norm_q, (size_t)l * D), w.rope_cos, w.rope_sin, W(blk, L.qrot), D, M, c.S, D, c.eps_qk, st, 1,
                                 qkv + D, P(w.norm_k, (size_t)l * D), W(blk, L.krot)));  // q and k in one launch
        // 5. self-attention
        FTMI_TRY(attn_fwd(self_attn_args(c, L, blk), st));
        // 6. to_out (+ LoRA), gate * residual
        {
            GemmNtArgs a = linear_args(W(blk, L.o1), D, M, P(w.w_o, (size_t)l * D2), D, D, D, P(w.b_o, (size_t)l * D), W(blk, L.h1), D, V);
            a.epi = EPI_RESID; a.resid = h0; a.ldr = D; a.gate = ada + 2 * D; a.gate_bstride = ab; a.rows_per_batch = mg.rows;
            FTMI_TRY(proj(a, 3, 1, W(blk, L.xa_o)));
        }
        const bf16_t* h1 = W(blk, L.h1);
        // 7. cross-attention query (no pre-norm, no RoPE)
        {
            GemmNtArgs a = linear_args(h1, D, M, P(w.w_q2, (size_t)l * D2), D, D, D, P(w.b_q2, (size_t)l * D), W(blk, L.q2raw), D, V);
            FTMI_TRY(proj(a, 4, 1, W(blk, L.xa_q2)));
            FTMI_TRY(qknorm_rope_fwd(W(blk, L.q2raw), D, P(w.norm_q2, (size_t)l * D), nullptr, nullptr, W(blk, L.q2n), D, M, c.S, D, c.eps_qk, st));
        }
        // 9. cross-attention with the text-mask bias
        FTMI_TRY(attn_fwd(cross_attn_args(c, L, ws, blk, l, key_bias), st));
        // 10. to_out (+ LoRA), residual (no gate)
        {
            GemmNtArgs a = linear_args(W(blk, L.o2), D, M, P(w.w_o2, (size_t)l * D2), D, D, D, P(w.b_o2, (size_t)l * D), W(blk, L.h2), D, V);
            a.epi = EPI_RESID; a.resid = h1; a.ldr = D;
            FTMI_TRY(proj(a, 7, 1, W(blk, L.xa_o2)));
        }
        const bf16_t* h2 = W(blk, L.h2);
        // 11-13. norm2 + modulate, feed-forward, gate * residual
        FTMI_TRY(norm_modulate_fwd(h2, ada + 3 * D, ada + 7 * D, ab, W(ws, L.s_n2), M, mg.rows, D, c.eps_norm, 0, st));
        {
            GemmNtArgs a = linear_args(W(ws, L.s_n2), D, M, P(w.w_ff1, (size_t)l * c.D_ff * D), D, c.D_ff, D, P(w.b_ff1, (size_t)l * c.D_ff), W(ws, L.s_g), c.D_ff, V);
            a.out2 = W(blk, L.z); a.ldo2 = c.D_ff; a.epi = EPI_GELU;
            if (ff.on) FTMI_TRY(proj_with(a, ff.a1_sp + (size_t)l * 2 * r * D, ff.b1_ext + (size_t)l * c.D_ff * 3 * r, 1, W(blk, L.xa_ff1)));  // adapter 8: ff.net.0.proj
            else FTMI_TRY(gemm_nt(a, st));
        }
        {
            GemmNtArgs a = linear_args(W(ws, L.s_g), c.D_ff, M, P(w.w_ff2, (size_t)l * D * c.D_ff), c.D_ff, D, c.D_ff, P(w.b_ff2, (size_t)l * D), hout, D, V);
            a.epi = EPI_RESID; a.resid = h2; a.ldr = D; a.gate = ada + 5 * D; a.gate_bstride = ab; a.rows_per_batch = mg.rows;
            if (ff.on) FTMI_TRY(proj_with(a, ff.a2_sp + (size_t)l * 2 * r * c.D_ff, ff.b2_ext + (size_t)l * D * 3 * r, 1, W(blk, L.xa_ff2)));  // adapter 9: ff.net.2 (contracts over D_ff)
            else FTMI_TRY(gemm_nt(a, st));
        }
    }
    return 0;
}

// The forward's prologue comes in two parts.  The TEXT part depends on the prompt and the adapters only: the caption projection and the text-side k|v
// of every block with its LoRA extension and norm_k2 (kv2_all, k2n_all, xa_kv2_all).  The TIMESTEP part is the conditioning of `groups` timesteps, one
// row per modulation group (one per sample where every token of a sample shares its timestep).  A training step runs both (ltx_forward); the sampler runs
// the text part once per call and the timestep part once per denoising step (ltx_sample).
// The embedding MLP (sinusoid, two linears, the 6D linear) is small_linear's: 1-8 rows per launch, every row computed on its own, so more than 8 groups run
// in chunks of 8 and a row holds the bits it would hold in any other chunk (or alone).
static int ltx_time_embed(const ftmi_ltx_config& c, const ftmi_ltx_weights& w, const WsLayout& L, void* ws, const float* tvals, int groups, bf16_t* emb,
                          bf16_t* temb, hipStream_t st) {
    const int D = c.D;
    FTMI_TRY(timestep_sinusoid(tvals, W(ws, L.tsin), groups, st));
    for (int g0 = 0; g0 < groups; g0 += 8) {
        const int n = groups - g0 < 8 ? groups - g0 : 8;
        FTMI_TRY(small_linear(W(ws, L.tsin) + (size_t)g0 * 256, P(w.time_l1_w, 0), P(w.time_l1_b, 0), W(ws, L.t1) + (size_t)g0 * D, n, D, 256, 0, 0, st));
        FTMI_TRY(small_linear(W(ws, L.t1) + (size_t)g0 * D, P(w.time_l2_w, 0), P(w.time_l2_b, 0), emb + (size_t)g0 * D, n, D, D, 1, 0, st));
        FTMI_TRY(small_linear(emb + (size_t)g0 * D, P(w.time_lin_w, 0), P(w.time_lin_b, 0), temb + (size_t)g0 * 6 * D, n, 6 * D, D, 1, 0, st));
    }
    return 0;
}
static int ltx_ada_tables(const ftmi_ltx_config& c, const ftmi_ltx_weights& w, const WsLayout& L, void* ws, int groups, hipStream_t st) {
    FTMI_TRY(ada_prep(P(w.tables, 0), W(ws, L.temb), W(ws, L.ada), c.L, groups, c.D, st));
    FTMI_TRY(ada_out_prep(P(w.table_out, 0), W(ws, L.emb), W(ws, L.ada_out), groups, c.D, st));
    return 0;
}
static int ltx_prologue_time(const ftmi_ltx_config& c, const ftmi_ltx_weights& w, const WsLayout& L, void* ws, const float* tvals, int groups, hipStream_t st) {
    FTMI_TRY(ltx_time_embed(c, w, L, ws, tvals, groups, W(ws, L.emb), W(ws, L.temb), st));
    return ltx_ada_tables(c, w, L, ws, groups, st);
}

static int ltx_prologue_text(const ftmi_ltx_config& c, const ftmi_ltx_weights& w, const WsLayout& L, void* ws, const bf16_t* text, hipStream_t st) {
    const int Mt = c.B * c.T, D = c.D, r = c.r, V = c.gemm_variant;
    const float s = c.lora_scale;
    // ---- caption projection ----
    {
        GemmNtArgs a = linear_args(text, c.D_cap, Mt, P(w.cap_l1_w, 0), c.D_cap, D, c.D_cap, P(w.cap_l1_b, 0), W(ws, L.cap_h), D, V);
        a.epi = EPI_GELU;
        FTMI_TRY(gemm_nt(a, st));
        FTMI_TRY(gemm_nt(linear_args(W(ws, L.cap_h), D, Mt, P(w.cap_l2_w, 0), D, D, D, P(w.cap_l2_b, 0), W(ws, L.e), D, V), st));
    }
    const bf16_t* e = W(ws, L.e);

    // ---- cross-attention keys/values of EVERY block (the text stream does not change across blocks) ----
    {
        // the k | v adapters of all L blocks as 2L adapters on the one input e
        GemmNtArgs a = linear_args(e, D, Mt, P(w.w_kv2, 0), D, c.L * 2 * D, D, P(w.b_kv2, 0), W(ws, L.kv2_all), (long)c.L * 2 * D, V);
        if (r > 0) {
            // XA[:, (l,k|v)] = s * e A_{l,k|v}^T : adapters 5,6 of block l are 2 * 2r consecutive plane rows, blocks 8 * 2r * D apart
            GemmNtArgs x = lora_down_args(e, D, Mt, P(w.lora_a_sp, 5L * 2 * r * D), 2 * c.L, D, r, s, W(ws, L.xa_kv2_all));
            x.w_grp_n = 4 * r; x.w_grp_stride = 16L * r * D; x.variant = V;
            FTMI_TRY(gemm_nt(x, st));
            lora_ext_fwd(a, W(ws, L.xa_kv2_all), 2 * c.L, r, P(w.lora_b_ext, 5L * D * 3 * r));
            a.w2_grp_n = 2 * D; a.w2_grp_stride = 8L * D * 3 * r;
        }
        FTMI_TRY(gemm_nt(a, st));
        // k2 = norm_k(k2raw): rows ordered (token, block): row i = t * L + l reads kv2_all + i * 2D, weight row l
        FTMI_TRY(qknorm_rope_fwd(W(ws, L.kv2_all), 2 * D, P(w.norm_k2, 0), nullptr, nullptr, W(ws, L.k2n_all), D, Mt * c.L, Mt * c.L, D,
                                 c.eps_qk, st, c.L));
    }
    return 0;
}

static int ltx_proj_in(const ftmi_ltx_config& c, const ftmi_ltx_weights& w, const WsLayout& L, void* ws, const bf16_t* x_t, hipStream_t st) {
    return gemm_nt(linear_args(x_t, c.C_in, c.B * c.S, P(w.proj_in_w, 0), c.C_in, c.D, c.C_in, P(w.proj_in_b, 0), W(ws, L.hs), c.D, c.gemm_variant), st);
}

// The block stack and the tail (LayerNorm + modulate + proj_out) over a prepared workspace: hs[0], the conditioning and the text-side k|v are in place.
static int ltx_blocks_tail(const ftmi_ltx_config& c, const ftmi_ltx_weights& w, const FfOps& ff, const WsLayout& L, void* ws, const float* key_bias, bf16_t* pred,
                           hipStream_t st, const ModGroups& mg) {
    const int M = c.B * c.S, D = c.D, V = c.gemm_variant;
    FuseCtx fx{reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + L.sk_flags), 0};
    if (hipMemsetAsync(fx.flags, 0, 4096, st) != hipSuccess) return set_error(FTMI_ERR_LAUNCH, "ltx_forward: memset of the row-tile counters failed");
    for (int l = 0; l < c.L; ++l) FTMI_TRY(ltx_block_forward(c, w, ff, L, ws, l, key_bias, st, fx, mg));

    // ---- tail: LayerNorm + modulate + proj_out ----
    const bf16_t* hL = W(ws, L.hs) + (size_t)c.L * M * D;
    const bf16_t* ao = W(ws, L.ada_out);
    FTMI_TRY(norm_modulate_fwd(hL, ao, ao + 2 * D, 3L * D, W(ws, L.s_ln), M, mg.rows, D, c.eps_norm, 1, st));
    FTMI_TRY(gemm_nt(linear_args(W(ws, L.s_ln), D, M, P(w.proj_out_w, 0), D, c.C_out, D, P(w.proj_out_b, 0), pred, c.C_out, V), st));
    return 0;
}

int ltx_forward(const ftmi_ltx_config& c, const ftmi_ltx_ff_weights& w, const bf16_t* x_t, const bf16_t* text, const float* key_bias, const float* sigma,
                bf16_t* pred, void* ws, size_t ws_bytes, hipStream_t st) {
    FTMI_TRY(check_cfg(c));
    struct ValidWidth {  // (normalisations of a zero-padded narrow model take their mean over d_valid channels; reset when the pass has queued its launches)
        explicit ValidWidth(int dv) { rowwise_set_valid_width(dv); }
        ~ValidWidth() { rowwise_set_valid_width(0); }
    } valid_width_guard(c.d_valid);
    FfOps ff;
    FTMI_TRY(ff_ops(c, w, &ff));
    const WsLayout L = make_layout(c, 0, ff.on);
    if (ws_bytes < L.total) return set_error(FTMI_ERR_INVALID, "ltx_forward: workspace too small");
    FTMI_TRY(ltx_prologue_time(c, w.base, L, ws, sigma, c.B, st));
    FTMI_TRY(ltx_proj_in(c, w.base, L, ws, x_t, st));
    FTMI_TRY(ltx_prologue_text(c, w.base, L, ws, text, st));
    return ltx_blocks_tail(c, w.base, ff, L, ws, key_bias, pred, st, ModGroups{c.B, c.S});
}

// ---- forward with one timestep per latent frame (forward only) -----------------------------------------------------------------------------------
// timesteps fp32 [B, frames]: tokens [f S / frames, (f + 1) S / frames) of sample b are modulated by the conditioning of timesteps[b][f].  The tables are
// [L][B frames][8][D] / [B frames][3][D]; norm_modulate_fwd and the gated-residual GEMM epilogues pick row (token row) / (S / frames) of them -- every output
// row by its own index, in every kernel nt_route() can choose (gemm_nt_kernel and nt16_body compute m / rows_per_batch per lane: there is no per-tile gate).
// Attention, RoPE and the text side see the true batch.  Workspace: the checkpoint = 1 layout with the taller tables; nothing is kept for a backward.
static ftmi_ltx_config frames_cfg(const ftmi_ltx_config& c) {
    ftmi_ltx_config fc = c;
    fc.checkpoint = 1;
    return fc;
}
size_t ltx_forward_frames_workspace_bytes(const ftmi_ltx_config& c, const ftmi_ltx_ff_weights& w, int frames) {
    FfOps ff;
    return ff_ops(c, w, &ff) == 0 && frames > 0 ? make_layout(frames_cfg(c), c.B * frames, ff.on).total : 0;
}
int ltx_forward_frames(const ftmi_ltx_config& c0, const ftmi_ltx_ff_weights& w, const bf16_t* x_t, const bf16_t* text, const float* key_bias,
                       const float* timesteps, int frames, bf16_t* pred, void* ws, size_t ws_bytes, hipStream_t st) {
    if (frames <= 0) return set_error(FTMI_ERR_INVALID, "ltx_forward_frames: frames must be positive");
    if (c0.d_valid || c0.head_dim_valid) return set_error(FTMI_ERR_UNSUPPORTED, "ltx_forward_frames: narrow (zero-padded) geometries are not supported");
    const ftmi_ltx_config c = frames_cfg(c0);
    FTMI_TRY(check_cfg(c, frames));
    const int G = c.B * frames;
    FfOps ff;
    FTMI_TRY(ff_ops(c, w, &ff));
    const WsLayout L = make_layout(c, G, ff.on);
    if (ws_bytes < L.total) return set_error(FTMI_ERR_INVALID, "ltx_forward_frames: workspace too small");
    FTMI_TRY(ltx_prologue_time(c, w.base, L, ws, timesteps, G, st));
    FTMI_TRY(ltx_proj_in(c, w.base, L, ws, x_t, st));
    FTMI_TRY(ltx_prologue_text(c, w.base, L, ws, text, st));
    return ltx_blocks_tail(c, w.base, ff, L, ws, key_bias, pred, st, ModGroups{G, c.S / frames});
}

// ---- latent sampling: the whole denoising loop as one call, zero host syncs -------------------------------------------------------------------------
// The model runs at batch nb = 2B (rows [0, B) unconditional, [B, 2B) conditional) or B (guidance == 1) over the checkpoint = 1 workspace layout -- one
// block slot plus the residual stream, nothing kept for a backward -- followed by the sampler's own buffers.
struct SampleLayout {
    ftmi_ltx_config mc;  // the model's configuration: batch nb, checkpoint = 1
    WsLayout L;
    size_t xin, pred, text, kbias, tval, total;
    size_t emb2, temb2;  // conditioned sampling (frames > 0): the embedding rows of the two distinct timesteps of a step, [2][D] and [2][6D] (row 0: timestep 0)
};
static SampleLayout make_sample_layout(const ftmi_ltx_config& c, int two_pass, int frames = 0, bool ff = false) {
    SampleLayout s;
    s.mc = c;
    s.mc.B = c.B * (two_pass ? 2 : 1);
    s.mc.checkpoint = 1;
    s.L = make_layout(s.mc, frames > 0 ? s.mc.B * frames : 0, ff);
    Bump g;
    g.off = s.L.total;
    const size_t nb = (size_t)s.mc.B;
    s.xin = g.take(nb * c.S * c.C_in * 2);
    s.pred = g.take(nb * c.S * c.C_out * 2);
    s.text = g.take(nb * c.T * c.D_cap * 2);
    s.kbias = g.take(nb * c.T * 4);
    s.tval = g.take((frames > 0 ? nb * frames : nb) * 4);
    s.emb2 = s.temb2 = 0;
    if (frames > 0) {
        s.emb2 = g.take(2 * (size_t)c.D * 2);
        s.temb2 = g.take(2 * 6 * (size_t)c.D * 2);
    }
    s.total = g.off;
    return s;
}

size_t ltx_sample_workspace_bytes(const ftmi_ltx_config& c, const ftmi_ltx_ff_weights& w, int two_pass) {
    FfOps ff;
    return ff_ops(c, w, &ff) == 0 ? make_sample_layout(c, two_pass, 0, ff.on).total : 0;
}
size_t ltx_sample_cond_workspace_bytes(const ftmi_ltx_config& c, const ftmi_ltx_ff_weights& w, int two_pass, int frames) {
    FfOps ff;
    return ff_ops(c, w, &ff) == 0 && frames > 0 ? make_sample_layout(c, two_pass, frames, ff.on).total : 0;
}

// FTMI_SAMPLE_HOIST=0 (read once; ftmi_reload_switches() re-reads it) repeats the text part of the prologue in every step, as a loop over ltx_forward
// does: the A/B partner of the measurement in DESIGN.md section 7, same bits.
//
// frames > 0: conditioned (image-to-video) sampling, ltx_sample_cond.  Restates [upstream, unpinned] LTXImageToVideoPipeline.__call__: the first
// cond_frames latent frames of every sample of x are clean conditioning latents -- the model sees timestep 0 on them and timesteps[i] on the other frames
// (t * (1 - conditioning_mask)), the guidance combine and the Euler update touch the other frames only.  The conditioning tables have one row per
// (model row, frame).  A step knows two distinct timesteps only, so the embedding MLP runs on ONE row per step (the live timestep); the timestep-0 row is
// computed once per call, next to the text hoist, and cond_rows_expand deals the two rows out to the groups.  With FTMI_SAMPLE_HOIST=0 every step runs the
// whole per-frame prologue of ltx_forward_frames instead (all groups through the MLP): same bits, a row's embedding does not depend on its neighbours.
static int ltx_sample_impl(const ftmi_ltx_config& c, const ftmi_ltx_ff_weights& w, const bf16_t* text_cond, const bf16_t* text_uncond, const float* kbias_cond,
                           const float* kbias_uncond, float* x, const float* sigmas, const float* timesteps, int n_steps, float guidance, int frames,
                           int cond_frames, void* ws, size_t ws_bytes, hipStream_t st) {
    static const EnvSwitch hoist_sw("FTMI_SAMPLE_HOIST", 1);
    const int hoist = hoist_sw.get();
    const int two_pass = guidance != 1.0f;
    if (n_steps <= 0) return set_error(FTMI_ERR_INVALID, "ltx_sample: no steps");
    if (c.B <= 0 || c.B * (two_pass ? 2 : 1) > 8) return set_error(FTMI_ERR_UNSUPPORTED, "ltx_sample: at most 4 videos with guidance, 8 without (model batch <= 8)");
    if (c.C_in != c.C_out) return set_error(FTMI_ERR_INVALID, "ltx_sample: the model's output is fed back as its input: C_in must equal C_out");
    if (c.d_valid || c.head_dim_valid) return set_error(FTMI_ERR_UNSUPPORTED, "ltx_sample: narrow (zero-padded) geometries are not supported");
    if (frames > 0 && (cond_frames < 0 || cond_frames > frames)) return set_error(FTMI_ERR_INVALID, "ltx_sample_cond: cond_frames must lie in [0, frames]");
    if (frames > 0 && c.C_in % 8) return set_error(FTMI_ERR_UNSUPPORTED, "ltx_sample_cond: the channel count must be a multiple of 8 (the held prefix moves in 16-byte vectors)");
    FfOps ff;
    FTMI_TRY(ff_ops(c, w, &ff));
    const SampleLayout sl = make_sample_layout(c, two_pass, frames, ff.on);
    const ftmi_ltx_config& mc = sl.mc;
    FTMI_TRY(check_cfg(mc, frames));
    if (ws_bytes < sl.total) return set_error(FTMI_ERR_INVALID, "ltx_sample: workspace too small");
    const WsLayout& L = sl.L;
    const int B = c.B, nb = mc.B;
    const ModGroups mg = frames > 0 ? ModGroups{nb * frames, c.S / frames} : ModGroups{nb, c.S};
    const long per_sample = (long)c.S * c.C_in;
    const long hold = frames > 0 ? (long)cond_frames * (c.S / frames) * c.C_in : 0;  // the held prefix of every sample, in elements
    bf16_t* xin = W(ws, sl.xin);
    bf16_t* pred = W(ws, sl.pred);
    bf16_t* text = W(ws, sl.text);
    float* tval = WF(ws, sl.tval);
    const float* kbias = nullptr;

    // rows [0, B) unconditional, [B, 2B) conditional: one text tensor / one bias tensor for the batched model call
    const size_t tbytes = (size_t)B * c.T * c.D_cap * 2, kbytes = (size_t)B * c.T * 4;
    bool ok = true;
    if (two_pass) {
        ok = ok && hipMemcpyAsync(text, text_uncond, tbytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(reinterpret_cast<char*>(text) + tbytes, text_cond, tbytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
        if (kbias_cond) {
            float* kb = WF(ws, sl.kbias);
            ok = ok && hipMemcpyAsync(kb, kbias_uncond, kbytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(kb + (size_t)B * c.T, kbias_cond, kbytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
            kbias = kb;
        }
    } else {
        ok = ok && hipMemcpyAsync(text, text_cond, tbytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
        kbias = kbias_cond;
    }
    if (!ok) return set_error(FTMI_ERR_LAUNCH, "ltx_sample: copy of the prompt embeddings failed");

    if (hoist) FTMI_TRY(ltx_prologue_text(mc, w.base, L, ws, text, st));
    bf16_t* emb2 = frames > 0 ? W(ws, sl.emb2) : nullptr;
    bf16_t* temb2 = frames > 0 ? W(ws, sl.temb2) : nullptr;
    if (frames > 0 && hoist) {  // the timestep-0 row of the conditioning: constant over the loop
        if (hipMemsetAsync(tval, 0, 4, st) != hipSuccess) return set_error(FTMI_ERR_LAUNCH, "ltx_sample_cond: memset of the timestep failed");
        FTMI_TRY(ltx_time_embed(mc, w.base, L, ws, tval, 1, emb2, temb2, st));
    }
    FTMI_TRY(cfg_euler_step(nullptr, x, nullptr, nullptr, 0, guidance, xin, B, per_sample, st));  // the first model input: bf16(x) in every half
    for (int i = 0; i < n_steps; ++i) {
        if (frames <= 0) {
            FTMI_TRY(bcast_f32(timesteps + i, tval, nb, st));
            FTMI_TRY(ltx_prologue_time(mc, w.base, L, ws, tval, nb, st));
        } else if (hoist) {
            FTMI_TRY(ltx_time_embed(mc, w.base, L, ws, timesteps + i, 1, emb2 + mc.D, temb2 + 6 * (size_t)mc.D, st));
            FTMI_TRY(cond_rows_expand(emb2, temb2, W(ws, L.emb), W(ws, L.temb), mg.n, frames, cond_frames, mc.D, st));
            FTMI_TRY(ltx_ada_tables(mc, w.base, L, ws, mg.n, st));
        } else {
            FTMI_TRY(frame_timesteps(timesteps + i, tval, mg.n, frames, cond_frames, st));
            FTMI_TRY(ltx_prologue_time(mc, w.base, L, ws, tval, mg.n, st));
        }
        FTMI_TRY(ltx_proj_in(mc, w.base, L, ws, xin, st));
        if (!hoist) FTMI_TRY(ltx_prologue_text(mc, w.base, L, ws, text, st));
        FTMI_TRY(ltx_blocks_tail(mc, w.base, ff, L, ws, kbias, pred, st, mg));
        FTMI_TRY(cfg_euler_step(pred, x, sigmas + i, sigmas + i + 1, 0, guidance, i + 1 < n_steps ? xin : nullptr, B, per_sample, st, hold));
    }
    return 0;
}

int ltx_sample(const ftmi_ltx_config& c, const ftmi_ltx_ff_weights& w, const bf16_t* text_cond, const bf16_t* text_uncond, const float* kbias_cond,
               const float* kbias_uncond, float* x, const float* sigmas, const float* timesteps, int n_steps, float guidance, void* ws, size_t ws_bytes,
               hipStream_t st) {
    return ltx_sample_impl(c, w, text_cond, text_uncond, kbias_cond, kbias_uncond, x, sigmas, timesteps, n_steps, guidance, 0, 0, ws, ws_bytes, st);
}

int ltx_sample_cond(const ftmi_ltx_config& c, const ftmi_ltx_ff_weights& w, const bf16_t* text_cond, const bf16_t* text_uncond, const float* kbias_cond,
                    const float* kbias_uncond, float* x, const float* sigmas, const float* timesteps, int n_steps, float guidance, int frames,
                    int cond_frames, void* ws, size_t ws_bytes, hipStream_t st) {
    if (frames <= 0) return set_error(FTMI_ERR_INVALID, "ltx_sample_cond: frames must be positive");
    return ltx_sample_impl(c, w, text_cond, text_uncond, kbias_cond, kbias_uncond, x, sigmas, timesteps, n_steps, guidance, frames, cond_frames, ws, ws_bytes, st);
}

// Backward of blocks [l_lo, l_hi) in descending order (the tail first when l_hi == L).  When the call returns (stream order) the LoRA
// gradients of exactly those blocks are FINAL -- all 8 adapters, the text-side ones included -- so a data-parallel caller can start
// the gradient exchange of that block range while the next call computes the blocks below it (DDP's bucketed overlap,
// finetrainers/parallel/ptd.py:462-463, without a reducer).  State between calls lives in the workspace; l_hi..l_lo must tile L..0.
int ltx_backward_range(const ftmi_ltx_config& c, const ftmi_ltx_ff_weights& w, const bf16_t* text, const float* key_bias, const bf16_t* dpred, float* grad_a,
                       float* grad_b, float* grad_ff, void* ws, size_t ws_bytes, int l_hi, int l_lo, int accumulate, hipStream_t st) {
    (void)text;
    FTMI_TRY(check_cfg(c));
    struct ValidWidth {  // (normalisations of a zero-padded narrow model take their mean over d_valid channels; reset when the pass has queued its launches)
        explicit ValidWidth(int dv) { rowwise_set_valid_width(dv); }
        ~ValidWidth() { rowwise_set_valid_width(0); }
    } valid_width_guard(c.d_valid);
    FfOps ff;
    FTMI_TRY(ff_ops(c, w, &ff));
    if (ff.on && !grad_ff) return set_error(FTMI_ERR_INVALID, "ltx_backward: feed-forward adapters without their gradient buffer");
    const WsLayout L = make_layout(c, 0, ff.on);
    if (ws_bytes < L.total) return set_error(FTMI_ERR_INVALID, "ltx_backward: workspace too small");
    const size_t ff_per_block = 2 * (size_t)c.r * ((size_t)c.D + c.D_ff);  // [A1 r D | B1 F r | A2 r F | B2 D r]
    if (l_lo < 0 || l_hi > c.L || l_lo >= l_hi) return set_error(FTMI_ERR_INVALID, "ltx_backward: bad block range");
    if (c.r > 0 && !accumulate && l_hi == c.L) {  // .grad was None: the weight-gradient kernels accumulate (split-token atomics), so start from zero
        const size_t nbytes = (size_t)c.L * 8 * c.r * c.D * sizeof(float);
        if (hipMemsetAsync(grad_a, 0, nbytes, st) != hipSuccess || hipMemsetAsync(grad_b, 0, nbytes, st) != hipSuccess)
            return set_error(FTMI_ERR_LAUNCH, "ltx_backward: memset of the gradient buffer failed");
        if (ff.on && hipMemsetAsync(grad_ff, 0, (size_t)c.L * ff_per_block * sizeof(float), st) != hipSuccess)
            return set_error(FTMI_ERR_LAUNCH, "ltx_backward: memset of the feed-forward gradient buffer failed");
    }
    const int M = c.B * c.S, Mt = c.B * c.T, D = c.D, r = c.r, V = c.gemm_variant;
    const long D2 = (long)D * D;
    const float s = c.lora_scale;
    const bf16_t* e = W(ws, L.e);

    bf16_t* dh[2] = {W(ws, L.s_dh0), W(ws, L.s_dh1)};
    bf16_t* d1 = W(ws, L.s_d1);
    bf16_t* d2 = W(ws, L.s_d2);
    bf16_t* dO = W(ws, L.s_d3);

    // ---- tail ----
    if (l_hi == c.L) {
        FTMI_TRY(gemm_nt(linear_args(dpred, c.C_out, M, P(w.base.proj_out_w_t, 0), c.C_out, D, c.C_out, nullptr, d1, D, V), st));
        const bf16_t* hL = W(ws, L.hs) + (size_t)c.L * M * D;
        const bf16_t* ao = W(ws, L.ada_out);
        // the gated copy bf(dh * gate_mlp) that opens the last block's backward is written by the same kernel (into dO, idle here)
        const bf16_t* ada_last = W(ws, L.ada) + (size_t)(c.L - 1) * c.B * 8 * D;
        FTMI_TRY(norm_modulate_bwd(hL, d1, ao + 2 * D, 3L * D, nullptr, dh[0], M, c.S, D, c.eps_norm, 1, st, ada_last + 5 * D, 8L * D, dO));
    }
    int cur = (c.L - l_hi) & 1;  // the gradient of the residual stream ping-pongs between two buffers, one flip per finished block

    // LoRA adapter backward, critical-path half: dXA = s * dY B (needed at once by the dgrad K-extension).  The weight
    // gradients dB += dY^T XA and dA += dXA^T X only feed the gradient buffer, so dY / dXA are kept per block and all 28
    // blocks of one adapter are reduced by ONE batched launch after the loop (fills the GPU instead of 28 latency-bound ones).
    auto lora_dxa = [&](const bf16_t* dY, long lddy, int rows, int nadp, int adp, int l, bf16_t* dxa_out) -> GemmNtArgs {
        const bf16_t* lbt = P(w.base.lora_bt_sp, ((size_t)l * 8 + adp) * 2 * r * D);  // [nadp * 2r][D]: (hi, lo) planes of B^T
        return lora_down_args(dY, lddy, rows, lbt, nadp, D, r, s, dxa_out, nadp > 1 ? D : 0);
    };
    FuseCtx fx{reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + L.sk_flags), 0};  // row-tile counters of the fused down-projection + GEMM launches of this call
    if (r > 0 && hipMemsetAsync(fx.flags, 0, 4096, st) != hipSuccess) return set_error(FTMI_ERR_LAUNCH, "ltx_backward: memset of the row-tile counters failed");

    // LoRA weight gradients dB += dY^T XA, dA += dXA^T X only feed the gradient buffer: ONE batched launch per adapter group over all
    // blocks of this call's range, after its block loop (fills the GPU instead of 28 latency-bound launches per adapter).
    auto lora_wgrad = [&](int l0, int nb, hipStream_t s2) -> int {
        char* blk0 = reinterpret_cast<char*>(ws) + L.blk0 + L.blk_stride * l0;
        const long bs = (long)(L.blk_stride / 2);  // block stride in bf16 elements
        struct G { size_t dy; long lddy; int rows, nadp, adp; size_t xa, dxa; const bf16_t* x; long ldx, x_bs; };
        const G groups[4] = {
            {L.g_o2, D, M, 1, 7, L.xa_o2, L.dxa_o2, W(blk0, L.o2), D, bs},
            {L.g_q2, D, M, 1, 4, L.xa_q2, L.dxa_q2, W(blk0, L.h1), D, bs},
            {L.g_o, D, M, 1, 3, L.xa_o, L.dxa_o, W(blk0, L.o1), D, bs},
            {L.g_qkv, 3L * D, M, 3, 0, L.xa_qkv, L.dxa_qkv, W(blk0, L.n1), D, bs},
        };
        float* ga = grad_a + (size_t)l0 * 8 * r * D;
        float* gb = grad_b + (size_t)l0 * 8 * D * r;
        for (const G& gr : groups) {
            GemmTnArgs t = lora_db_args(W(blk0, gr.dy), gr.lddy, W(blk0, gr.xa), gr.nadp, r, D, gb + (size_t)gr.adp * D * r, gr.rows);  // dB[l] += dY[l]^T XA[l]
            tn_batch(t, nb, bs, bs, 8L * D * r);
            FTMI_TRY(gemm_tn(t, s2));
            GemmTnArgs u = lora_da_args(W(blk0, gr.dxa), gr.nadp, r, gr.x, gr.ldx, D, ga + (size_t)gr.adp * r * D, gr.rows);  // dA[l] += dXA[l]^T X[l]
            tn_batch(u, nb, bs, gr.x_bs, 8L * r * D);
            FTMI_TRY(gemm_tn(u, s2));
        }
        return 0;
    };
    for (int l = l_hi - 1; l >= l_lo; --l) {
        char* blk = reinterpret_cast<char*>(ws) + L.blk0 + L.blk_stride * l;
        const bf16_t* h0 = W(ws, L.hs) + (size_t)l * M * D;
        const bf16_t* ada = W(ws, L.ada) + (size_t)l * c.B * 8 * D;
        const long ab = 8L * D;
        const bf16_t* lat = w.base.lora_at_ext ? P(w.base.lora_at_ext, (size_t)l * 8 * D * 3 * r) : nullptr;  // [8][D][3r]  [A^T_hi | A^T_hi | A^T_lo]
        const bf16_t* h1 = W(blk, L.h1);
        const bf16_t* h2 = W(blk, L.h2);
        const bf16_t* dhin = dh[cur];
        // the input gradient `a` of a projection (a.X = dY) + dXA A of its adapters adp .. adp + nadp - 1, at_ext [D, 3 nadp r]; dxa is kept for dA
        auto proj_bwd = [&](GemmNtArgs& a, int adp, int nadp, bf16_t* dxa, const bf16_t* at_ext) -> int {
            if (r <= 0) return gemm_nt(a, st);
            lora_ext_bwd(a, dxa, nadp, r, at_ext, 3L * nadp * r);
            return lora_gemm(a, lora_dxa(a.X, a.ldx, M, nadp, adp, l, dxa), fx, st);
        };
        if (c.checkpoint) FTMI_TRY(ltx_block_forward(c, w.base, ff, L, ws, l, key_bias, st, fx, ModGroups{c.B, c.S}));  // the block's activations again, into the one slot

        // ---- feed-forward ----
        // (dO holds bf(dhin * gate_mlp): written by the kernel that produced dhin)
        const int F = c.D_ff;
        bf16_t* dz = W(ws, L.s_dbig);
        // the same for any operand pair: bt_sp = the (hi, lo) row planes of B^T [2r, a.K], at_ext [a.N, 3r] (the rectangular feed-forward adapters)
        auto proj_bwd_with = [&](GemmNtArgs& a, const bf16_t* bt_sp, const bf16_t* at_ext, bf16_t* dxa) -> int {
            lora_ext_bwd(a, dxa, 1, r, at_ext, 3L * r);
            return lora_gemm(a, lora_down_args(a.X, a.ldx, M, bt_sp, 1, a.K, r, s, dxa), fx, st);
        };
        if (ff.on && !c.checkpoint) {
            // n2 and g are scratch shared by all blocks (kept per block they would be 5.5 GB over 28 blocks at M = 5376): written again right before they are read.
            // Under checkpoint = 1 the recomputation pass above has just refilled both for this block.
            FTMI_TRY(norm_modulate_fwd(h2, ada + 3 * D, ada + 7 * D, ab, W(ws, L.s_n2), M, c.S, D, c.eps_norm, 0, st));
            FTMI_TRY(gelu_from_pre(W(blk, L.z), F, W(ws, L.s_g), F, M, F, st));
        }
        {   // dz = (dO W2 [+ dXA2 A2]) * gelu'(z)
            GemmNtArgs a = linear_args(dO, D, M, P(w.base.w_ff2_t, (size_t)l * F * D), D, F, D, nullptr, dz, F, V);
            a.epi = EPI_DGELU; a.aux = W(blk, L.z); a.ldaux = F;
            if (ff.on) FTMI_TRY(proj_bwd_with(a, ff.b2t_sp + (size_t)l * 2 * r * D, ff.a2t_ext + (size_t)l * F * 3 * r, W(ws, L.s_dxa_ff2)));
            else FTMI_TRY(gemm_nt(a, st));
        }
        {   // dn2 = dz W1 [+ dXA1 A1]
            GemmNtArgs a = linear_args(dz, F, M, P(w.base.w_ff1_t, (size_t)l * D * F), F, D, F, nullptr, d2, D, V);
            if (ff.on) FTMI_TRY(proj_bwd_with(a, ff.b1t_sp + (size_t)l * 2 * r * F, ff.a1t_ext + (size_t)l * D * 3 * r, W(ws, L.s_dxa_ff1)));
            else FTMI_TRY(gemm_nt(a, st));
        }
        if (ff.on) {
            // the four feed-forward weight gradients of this block now, while dz and the gated dO are live (their operands are not kept per block; with P or Q =
            // D_ff = 8192 one launch is four times an attention adapter's: no longer latency-sized)
            float* g0 = grad_ff + (size_t)l * ff_per_block;
            float *gA1 = g0, *gB1 = gA1 + (size_t)r * D, *gA2 = gB1 + (size_t)F * r, *gB2 = gA2 + (size_t)r * F;
            FTMI_TRY(gemm_tn(lora_db_args(dO, D, W(blk, L.xa_ff2), 1, r, D, gB2, M), st));                    // dB2 += dO^T XA2
            FTMI_TRY(gemm_tn(lora_da_args(W(ws, L.s_dxa_ff2), 1, r, W(ws, L.s_g), F, F, gA2, M), st));        // dA2 += dXA2^T g
            FTMI_TRY(gemm_tn(lora_db_args(dz, F, W(blk, L.xa_ff1), 1, r, F, gB1, M), st));                    // dB1 += dz^T XA1
            FTMI_TRY(gemm_tn(lora_da_args(W(ws, L.s_dxa_ff1), 1, r, W(ws, L.s_n2), D, D, gA1, M), st));       // dA1 += dXA1^T n2
        }
        bf16_t* d3 = W(blk, L.g_o2);  // dh2: also the dY of attn2.to_out
        FTMI_TRY(norm_modulate_bwd(h2, d2, ada + 7 * D, ab, dhin, d3, M, c.S, D, c.eps_norm, 0, st));

        // ---- cross-attention ----
        {
            GemmNtArgs a = linear_args(d3, D, M, P(w.base.w_o2_t, (size_t)l * D2), D, D, D, nullptr, d1, D, V);
            FTMI_TRY(proj_bwd(a, 7, 1, W(blk, L.dxa_o2), lat + 7L * D * 3 * r));  // d1 = dO2
        }
        {
            AttnArgs a = cross_attn_args(c, L, ws, blk, l, key_bias);
            a.dout = d1;                  tok_strides(a.do_sb, a.do_sh, a.do_ss, c.S, D, 64);
            a.delta = WF(ws, L.s_delta);
            a.dq = d2;                    tok_strides(a.dq_sb, a.dq_sh, a.dq_ss, c.S, D, 64);
            a.dk = W(ws, L.g_k2n_all) + (size_t)l * D;            tok_strides(a.dk_sb, a.dk_sh, a.dk_ss, c.T, (long)c.L * D, 64);
            a.dv = W(ws, L.g_kv2_all) + (size_t)l * 2 * D + D;    tok_strides(a.dv_sb, a.dv_sh, a.dv_ss, c.T, (long)c.L * 2 * D, 64);
            FTMI_TRY(attn_bwd(a, st));
        }
        bf16_t* gq2 = W(blk, L.g_q2);  // dq2raw
        FTMI_TRY(qknorm_rope_bwd(W(blk, L.q2raw), D, P(w.base.norm_q2, (size_t)l * D), nullptr, nullptr, d2, D, gq2, D, M, c.S, D, c.eps_qk, st));
        {
            GemmNtArgs a = linear_args(gq2, D, M, P(w.base.w_q2_t, (size_t)l * D2), D, D, D, nullptr, d2, D, V);
            a.epi = EPI_RESID; a.resid = d3; a.ldr = D;
            a.out2 = W(blk, L.g_o); a.ldo2 = D; a.gate2 = ada + 2 * D; a.gate2_bstride = ab; a.rows_per_batch = c.S;  // go = bf(dh1 * gate_msa), fused
            FTMI_TRY(proj_bwd(a, 4, 1, W(blk, L.dxa_q2), lat + 4L * D * 3 * r));  // d2 = dh1
        }

        // ---- self-attention ----
        bf16_t* go = W(blk, L.g_o);  // d(attn1.to_out output)
        {
            GemmNtArgs a = linear_args(go, D, M, P(w.base.w_o_t, (size_t)l * D2), D, D, D, nullptr, dO, D, V);
            FTMI_TRY(proj_bwd(a, 3, 1, W(blk, L.dxa_o), lat + 3L * D * 3 * r));
        }
        bf16_t* dqkv = W(blk, L.g_qkv);
        const bf16_t* qkv = W(blk, L.qkv);
        {
            AttnArgs a = self_attn_args(c, L, blk);
            a.dout = dO;          tok_strides(a.do_sb, a.do_sh, a.do_ss, c.S, D, 64);
            a.delta = WF(ws, L.s_delta);
            a.dq = W(ws, L.s_dqr); tok_strides(a.dq_sb, a.dq_sh, a.dq_ss, c.S, D, 64);
            a.dk = W(ws, L.s_dkr); tok_strides(a.dk_sb, a.dk_sh, a.dk_ss, c.S, D, 64);
            a.dv = dqkv + 2 * D;   tok_strides(a.dv_sb, a.dv_sh, a.dv_ss, c.S, 3 * D, 64);
            FTMI_TRY(attn_bwd(a, st));
        }
        FTMI_TRY(qknorm_rope_bwd(qkv, 3 * D, P(w.base.norm_q, (size_t)l * D), w.base.rope_cos, w.base.rope_sin, W(ws, L.s_dqr), D, dqkv, 3 * D, M, c.S, D, c.eps_qk, st, 1,
                                 qkv + D, P(w.base.norm_k, (size_t)l * D), W(ws, L.s_dkr), dqkv + D));  // q and k in one launch
        if (r > 0 && l == 0) FTMI_TRY(gemm_nt(lora_dxa(dqkv, 3 * D, M, 3, 0, l, W(blk, L.dxa_qkv)), st));  // (block 0 has no input gradient: the dXA alone, for dA)
        if (l > 0) {
            GemmNtArgs a = linear_args(dqkv, 3 * D, M, P(w.base.w_qkv_t, (size_t)l * 3 * D2), 3 * D, D, 3 * D, nullptr, d1, D, V);
            FTMI_TRY(proj_bwd(a, 0, 3, W(blk, L.dxa_qkv), P(w.base.lora_at_qkv_ext, (size_t)l * D * 9 * r)));  // d1 = dn1
            const bf16_t* ada_prev = W(ws, L.ada) + (size_t)(l - 1) * c.B * 8 * D;  // the next block processed is l - 1
            FTMI_TRY(norm_modulate_bwd(h0, d1, ada + 6 * D, ab, d2, dh[cur ^ 1], M, c.S, D, c.eps_norm, 0, st, ada_prev + 5 * D, ab, dO));
            cur ^= 1;
        }
        if (c.checkpoint && r > 0) FTMI_TRY(lora_wgrad(l, 1, st));  // the slot is about to be reused: this block's weight gradients now
    }
    if (r > 0 && !c.checkpoint) FTMI_TRY(lora_wgrad(l_lo, l_hi - l_lo, st));
    const int nb = l_hi - l_lo;

    // ---- text side of the cross-attention, all blocks at once (nothing upstream of `e` needs a gradient) ----
    if (r > 0) {
        // d(k2raw) = RMSNorm backward of d(k2n); rows ordered (token, block) like the forward
        // (row i of this call = (token i / nb, block l_lo + i % nb): rows of one token are L apart in the all-block arrays)
        FTMI_TRY(qknorm_rope_bwd(W(ws, L.kv2_all) + (size_t)l_lo * 2 * D, 2 * D, P(w.base.norm_k2, (size_t)l_lo * D), nullptr, nullptr,
                                 W(ws, L.g_k2n_all) + (size_t)l_lo * D, D, W(ws, L.g_kv2_all) + (size_t)l_lo * 2 * D, 2 * D,
                                 Mt * nb, Mt * nb, D, c.eps_qk, st, nb, nullptr, nullptr, nullptr, nullptr, nb, c.L));
        // dXA[:, (l,k|v)] = s * dY[:, (l,k|v) slice] B_{l,k|v}: the 2 nb adapters of this range, written into their columns of the all-block array
        GemmNtArgs a = lora_down_args(W(ws, L.g_kv2_all) + (size_t)l_lo * 2 * D, (long)c.L * 2 * D, Mt, P(w.base.lora_bt_sp, ((size_t)l_lo * 8 + 5) * 2 * r * D), 2 * nb, D, r, s,
                                      W(ws, L.dxa_kv2_all) + (size_t)l_lo * 6 * r, D);
        a.w_grp_n = 4 * r; a.w_grp_stride = 16L * r * D; a.ldo = (long)c.L * 6 * r; a.variant = V;
        FTMI_TRY(gemm_nt(a, st));
    }

    // ---- LoRA weight gradients of the text-side adapters (all blocks in one launch each) ----
    if (r > 0) {
        {   // attn2.to_k / to_v: operands are column slices of the all-block arrays (batch stride = one block's columns)
            const long ldxa = (long)c.L * 6 * r;
            GemmTnArgs t = lora_db_args(W(ws, L.g_kv2_all) + (size_t)l_lo * 2 * D, (long)c.L * 2 * D, W(ws, L.xa_kv2_all) + (size_t)l_lo * 6 * r, 2, r, D,
                                        grad_b + ((size_t)l_lo * 8 + 5) * D * r, Mt);
            t.ldv = ldxa;
            tn_batch(t, nb, 2L * D, 6L * r, 8L * D * r);
            FTMI_TRY(gemm_tn(t, st));
            GemmTnArgs u = lora_da_args(W(ws, L.dxa_kv2_all) + (size_t)l_lo * 6 * r, 2, r, e, D, D, grad_a + ((size_t)l_lo * 8 + 5) * r * D, Mt);
            u.ldu = ldxa;
            tn_batch(u, nb, 6L * r, 0, 8L * r * D);
            FTMI_TRY(gemm_tn(u, st));
        }
    }
    return 0;
}

}  // namespace ftmi
