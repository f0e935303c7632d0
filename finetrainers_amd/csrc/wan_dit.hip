// Wan-T2V DiT block, forward / backward orchestrator for FULL fine-tuning and for LoRA fine-tuning over a frozen base: ONE C call per block and direction
// -- the unit FSDP-2 shards (finetrainers/parallel/ptd.py:466-499 wraps every block with fully_shard), so the sharder keeps interleaving its all-gathers
// and reduce-scatters between the calls.  Parameters arrive as the block's ONE flat bf16 buffer, gradients leave in ONE flat fp32 buffer of the same
// layout (finetrainers_amd/wan/block.py WanBlockLayout; the order is restated in Offsets below), activations live in a caller-owned `saved` buffer per
// block and transients in a `scratch` buffer shared by all blocks.
//
//   x [B, S, D] video tokens, enc [B, T, D] text tokens, mod fp32 [B, 6, D] = scale_shift_table + time projection (shift, scale, gate) x 2:
//     n1 = LN(x) * (1 + scale_msa) + shift_msa;  q|k|v = n1 W^T + b;  q, k <- RMSNorm across heads, rotary embedding;  o1 = attention(q, k, v)
//     x1 = x + gate_msa * (o1 W_o^T + b)
//     n2 = LN(x1; norm2);  q2 = n2 W^T + b;  k2|v2 = enc W^T + b;  q2, k2 <- RMSNorm;  o2 = attention(q2, k2, v2);  x2 = x1 + (o2 W_o2^T + b)
//     n3 = LN(x2) * (1 + scale_ff) + shift_ff;  out = x2 + gate_ff * (gelu_tanh(n3 W_1^T + b) W_2^T + b)
//
// Reference: [upstream] diffusers WanTransformerBlock / WanAttnProcessor2_0 as driven by finetrainers/models/wan/base_specification.py:433-493,
// restated in oracle/wan.py.  There is ONE walk per direction (block_forward / block_backward); the four entry points (wan_block_* for full fine-tuning,
// wan_lora_ffn_block_* for every LoRA configuration) differ in the context they hand it.  The kernel sequence is the one finetrainers_amd/wan/block.py (_block_forward / _block_backward) issues from Python, which stays as the second
// implementation (the tests compare the two bit for bit, what is summed with fp32 atomics up to their order).
//
// LoRA (the reference's Wan SFT recipes: --training_type lora, --target_modules "blocks.*(to_q|to_k|to_v|to_out.0)"): the base weights are FROZEN, fp32
// adapters A [8, r, D] / B [8, D, r] sit on the eight attention projections, in the order
//   0 attn1.to_q, 1 attn1.to_k, 2 attn1.to_v, 3 attn1.to_out.0, 4 attn2.to_q, 5 attn2.to_k, 6 attn2.to_v, 7 attn2.to_out.0
// and every projection computes y = x W^T + b + s (x A^T) B^T, s = alpha / r, through the NT GEMM's K-extension (attn1's q|k|v stay ONE N = 3D launch with
// three adapters on one input and attn2's k|v ONE N = 2D launch over the text rows, laid out as ltx_dit.hip's fused QKV).  The adapters are split into
// bf16 (hi, lo) planes once per call.  With r = 0 the walk issues the full fine-tune's launches, argument for argument.
//
// What the frozen base removes from the backward: the seven weight-gradient GEMMs, the bias / norm-weight / modulation / gate reductions (null
// reduction pointers), dmod, the seven weight transposes (K-contiguous twins arrive as pointers: the frozen base never invalidates them) and -- when
// denc == NULL, the text embedder being frozen too -- the [B T, 2D] x [2D, D] input-gradient GEMM into the text rows.
//
// saved (what the backward reads again), both modes:  n1, qkv, qn, kn, o1, lse1, x1, n2, q2, kv2, q2n, k2n, o2, lse2, x2, pre
//   full fine-tune, in addition: a1, n3, act, f -- read only by the gradients of gate_msa, W_1, W_2, gate_ff; the frozen base drops them: B S (3D + F) 2 bytes
//   r > 0, in addition: xa_qkv [M, 9r], xa_o1 [M, 3r], xa_q2 [M, 3r], xa_kv2 [Mt, 6r], xa_o2 [M, 3r]  (s x A^T as (hi | lo | hi) planes)
// scratch, full fine-tune (backward only): the seven transposed weights and the backward's transients.
// scratch, frozen base: forward transients (a1, n3, act, f, operand copies of A and B) overlaid with the backward's (+ dxa, operand copies of B^T and A^T).
// Launcher calls per block (an attention counts once): full fine-tune forward 19, backward 39.  Frozen base, r > 0: forward 2 splits + 5 down-projections
// + the full path's 19 = 26; backward 2 splits + 5 down-projections + 10 adapter-gradient GEMMs + 18 of the full path's 39 (its 7 transposes, 7
// weight-gradient GEMMs and 7 column sums are gone) = 35, 34 without denc.  With the feed-forward adapters: forward + 4 splits + 2 down-projections = 32 (the
// recomputation pass: 30 -- it runs net.2's down-projection, not its GEMM); backward + 4 splits + 2 down-projections + 4 adapter-gradient GEMMs = 45, 44
// without denc.
//
// Feed-forward adapters (the ftmi_wan_lora_ffn_block_* entries with cfg.ffn = 1; the reference hands --target_modules to peft unchanged, and a string that
// spells "ffn.net.0.proj|ffn.net.2" selects them -- its control trainer's default "...|ff.net.0.proj|ff.net.2" does NOT match Wan's "ffn"): two more adapters
// at the block's rank, rectangular,
//   ffn.net.0.proj  A_1 [r, D], B_1 [F, r]:  pre = n3 W_1^T + b_1 + XA_1 B_1^T and act = gelu(pre) in ONE launch (K-extension under the GELU epilogue);
//                                            dXA_1 = s dpre B_1 contracts over F;  dn3 = dpre W_1 + dXA_1 A_1
//   ffn.net.2       A_2 [r, F], B_2 [D, r]:  XA_2 = s act A_2^T contracts over F;  f = act W_2^T + b_2 + XA_2 B_2^T;
//                                            dpre = (df W_2 + dXA_2 A_2) * gelu'(pre) in ONE launch (K-extension under the GELU' epilogue)
// through the same proj_fwd / proj_bwd as the attention projections.  The four fp32 matrices arrive as pointers of their own (they are not [r, D] / [D, r]
// like the eight) and are split into the same (hi, lo) operand copies per call.  saved, in addition: xa_f1, xa_f2 [M, 3r] -- and n3 and act, which the frozen
// base otherwise drops: dA_1 += dXA_1^T n3 and dA_2 += dXA_2^T act read them.  They are KEPT, not recomputed: act is the GELU epilogue's rounding of an fp32
// accumulator, so recomputing its bits means running the [M, D] x [D, F] GEMM (and its down-projection) a second time in every backward, against
// B S (D + F) 2 bytes per block -- 426 MB at the recipe's bucket (20 280 tokens, D 1536, F 8960).  Gradient checkpointing brings that back to one block's
// worth: its recomputation pass refills n3, act, pre, xa_f1 with the identical launches and xa_f2 with net.2's down-projection alone.
//
// Image-to-video (Wan2.1-I2V: attn2 with added_kv_proj_dim; the same entries with cfg.TI > 0 image tokens enc_img [B, TI, D]): attn2 attends to a
// second, FROZEN key/value set  k_i = RMSNorm(enc_img W_ak^T + b), v_i = enc_img W_av^T + b  (one N = 2D GEMM and one RMSNorm over the B TI image rows) and
//   o2 = bf(attention(q2, k2, v2)) + bf(attention(q2, k_i, v_i))
// -- the second attention (attn_ctx2.hip) reads the first one's output and writes the sum, so the forward adds 3 launches (29) and the backward ONE (36): the
// image branch's dQ, which accumulates onto the text branch's.  No adapter sits on add_k_proj / add_v_proj / norm_added_k (the recipe's regex does not match
// them): they arrive in a separate flat buffer  W_ak | W_av [2D, D], b_ak | b_av [2D], norm_added_k [D]  and nothing flows back into them or into enc_img.
// (a second image, cfg.TI2 > 0 -- the first/last-frame model: its rows follow the first image's in enc_img, TI below then counts both and the two launches are
// attn_ctx2w_fwd / _dq, the wide pair)
// saved, in addition: kvi [B TI, 2D], kin [B TI, D], lse_i, o2s [B S, D] (the summed output: the input of to_out.0; o2 stays the text branch's own output,
// which its backward needs for rowsum(dO o O)).
#include "common.hip.h"
#include "kernels.h"
#include "lora_proj.hip.h"

namespace ftmi {

namespace {

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

// Every buffer of one call as a pointer, so that the walks never ask where a buffer lives.
struct Bufs {
    bf16_t *n1, *qkv, *qn, *kn, *o1, *a1, *x1, *n2, *q2, *kv2, *q2n, *k2n, *o2, *x2, *n3, *act, *pre, *f;  // activations
    float *lse1, *lse2;
    bf16_t *kvi, *kin, *o2s;                                             // image context of attn2 (zero-size at TI = 0)
    float* lse_i;
    bf16_t *xa_qkv, *xa_o1, *xa_q2, *xa_kv2, *xa_o2;                     // down-projected rows of the adapters (zero-size at r = 0)
    bf16_t *xa_f1, *xa_f2;                                               // ... of the feed-forward adapters (zero-size without them)
    bf16_t *a_sp, *b_ext;                                                // forward operand copies of the adapters
    bf16_t *f_a1_sp, *f_b1_ext, *f_a2_sp, *f_b2_ext;                     // ... of the feed-forward adapters: A_1 [2r, D], B_1 [F, 3r], A_2 [2r, F], B_2 [D, 3r]
    bf16_t *t_f2, *t_f1, *t_o2, *t_q2, *t_kv2, *t_o1, *t_qkv1;           // transposed weights (full fine-tune only)
    bf16_t *df, *dpre, *dn3, *dx2, *do2, *dkv2, *dq2n, *dk2n, *dq2, *dn2, *dx1, *da1, *do1, *dqkv, *dqn, *dkn, *dn1;  // backward transients
    float* delta;
    bf16_t *dxa, *bt_sp, *at_ext;                                        // backward down-projection and operand copies of the adapters
    bf16_t *f_b1t_sp, *f_a1t_ext, *f_b2t_sp, *f_a2t_ext;                 // ... of the feed-forward adapters: B_1^T [2r, F], A_1^T [D, 3r], B_2^T [2r, D], A_2^T [F, 3r]
    size_t saved_total, scratch_total;
};

// The plan of both buffers, resolved against their bases (the byte planners pass none and read the totals).  frozen: a1, n3, act and f are forward
// transients instead of saved activations, and the transposed weights are the caller's.  ffn (feed-forward adapters at the same rank): n3 and act stay
// saved, and everything the two adapters add is appended -- without them no offset moves.
Bufs make_layout(const ftmi_wan_block_config& c, int rank, bool frozen, void* saved = nullptr, void* scratch = nullptr, int TI = 0, bool ffn = false) {
    Bufs w;
    const size_t M = (size_t)c.B * c.S, Mt = (size_t)c.B * c.T, Mi = (size_t)c.B * (TI > 0 ? TI : 0), D = c.D, F = c.F, r = rank > 0 ? rank : 0, e2 = 2, stat = (size_t)c.B * c.H * c.S * 4;
    const size_t rf = ffn ? r : 0;
    Bump s, f, b;  // saved; scratch of the forward and of the backward, which overlay each other
    auto at = [](void* base, size_t off) { return reinterpret_cast<bf16_t*>(reinterpret_cast<uintptr_t>(base) + off); };
    auto S = [&](size_t bytes) { return at(saved, s.take(bytes)); };
    auto Fw = [&](size_t bytes) { return at(scratch, f.take(bytes)); };
    auto Bw = [&](size_t bytes) { return at(scratch, b.take(bytes)); };
    auto K = [&](size_t bytes) { return frozen ? Fw(bytes) : S(bytes); };                     // read again only by gradients of base parameters
    auto KF = [&](size_t bytes) { return ffn ? S(bytes) : K(bytes); };                        // ... and by the feed-forward adapters' dA
    auto T = [&](size_t bytes) { return frozen ? (bf16_t*)nullptr : Bw(bytes); };
    auto f32 = [](bf16_t* p) { return reinterpret_cast<float*>(p); };
    w.n1 = S(M * D * e2);
    w.qkv = S(M * 3 * D * e2);
    w.qn = S(M * D * e2);
    w.kn = S(M * D * e2);
    w.o1 = S(M * D * e2);
    w.lse1 = f32(S(stat));
    w.a1 = K(M * D * e2);
    w.x1 = S(M * D * e2);
    w.n2 = S(M * D * e2);
    w.q2 = S(M * D * e2);
    w.kv2 = S(Mt * 2 * D * e2);
    w.q2n = S(M * D * e2);
    w.k2n = S(Mt * D * e2);
    w.o2 = S(M * D * e2);
    w.lse2 = f32(S(stat));
    w.x2 = S(M * D * e2);
    w.n3 = KF(M * D * e2);
    w.act = KF(M * F * e2);
    w.pre = S(M * F * e2);
    w.f = K(M * D * e2);
    w.xa_qkv = S(M * 9 * r * e2);
    w.xa_o1 = S(M * 3 * r * e2);
    w.xa_q2 = S(M * 3 * r * e2);
    w.xa_kv2 = S(Mt * 6 * r * e2);
    w.xa_o2 = S(M * 3 * r * e2);
    w.kvi = S(Mi * 2 * D * e2);
    w.kin = S(Mi * D * e2);
    w.lse_i = f32(S(Mi ? stat : 0));
    w.o2s = S(Mi ? M * D * e2 : 0);
    w.xa_f1 = S(M * 3 * rf * e2);
    w.xa_f2 = S(M * 3 * rf * e2);
    w.saved_total = s.off;
    w.a_sp = Fw(8 * 2 * r * D * e2);
    w.b_ext = Fw(8 * D * 3 * r * e2);
    w.f_a1_sp = Fw(2 * rf * D * e2);
    w.f_b1_ext = Fw(F * 3 * rf * e2);
    w.f_a2_sp = Fw(2 * rf * F * e2);
    w.f_b2_ext = Fw(D * 3 * rf * e2);
    w.t_f2 = T(D * F * e2);
    w.t_f1 = T(D * F * e2);
    w.t_o2 = T(D * D * e2);
    w.t_q2 = T(D * D * e2);
    w.t_kv2 = T(2 * D * D * e2);
    w.t_o1 = T(D * D * e2);
    w.t_qkv1 = T(3 * D * D * e2);
    w.df = Bw(M * D * e2);
    w.dpre = Bw(M * F * e2);
    w.dn3 = Bw(M * D * e2);
    w.dx2 = Bw(M * D * e2);
    w.do2 = Bw(M * D * e2);
    w.dkv2 = Bw(Mt * 2 * D * e2);
    w.dq2n = Bw(M * D * e2);
    w.dk2n = Bw(Mt * D * e2);
    w.dq2 = Bw(M * D * e2);
    w.dn2 = Bw(M * D * e2);
    w.dx1 = Bw(M * D * e2);
    w.da1 = Bw(M * D * e2);
    w.do1 = Bw(M * D * e2);
    w.dqkv = Bw(M * 3 * D * e2);
    w.dqn = Bw(M * D * e2);
    w.dkn = Bw(M * D * e2);
    w.dn1 = Bw(M * D * e2);
    w.delta = f32(Bw(stat));
    w.dxa = Bw((M > Mt ? M : Mt) * 9 * r * e2);
    w.bt_sp = Bw(8 * 2 * r * D * e2);
    w.at_ext = Bw(D * 24 * r * e2);
    w.f_b1t_sp = Bw(2 * rf * F * e2);
    w.f_a1t_ext = Bw(D * 3 * rf * e2);
    w.f_b2t_sp = Bw(2 * rf * D * e2);
    w.f_a2t_ext = Bw(F * 3 * rf * e2);
    w.scratch_total = f.off > b.off ? f.off : b.off;
    return w;
}

int check_cfg(const ftmi_wan_block_config& c) {
    if (c.B <= 0 || c.S <= 0 || c.T <= 0) return set_error(FTMI_ERR_INVALID, "wan_block: empty problem");
    if (c.H * 128 != c.D || c.D % 128 != 0 || c.D > 5120) return set_error(FTMI_ERR_UNSUPPORTED, "wan_block: width must be heads x 128, at most 5120");
    if (c.F <= 0 || (c.F % 64)) return set_error(FTMI_ERR_UNSUPPORTED, "wan_block: the feed-forward width must be a multiple of 64");
    return 0;
}

ftmi_wan_block_config base_cfg(const ftmi_wan_lora_ffn_block_config& c) {
    ftmi_wan_block_config b;
    b.B = c.B; b.S = c.S; b.T = c.T; b.D = c.D; b.H = c.H; b.F = c.F; b.eps = c.eps; b.gemm_variant = c.gemm_variant;
    return b;
}

// every refusal of the LoRA block: the byte planners and both directions go through it
int check_lora_cfg(const ftmi_wan_lora_ffn_block_config& c) {
    FTMI_TRY(check_cfg(base_cfg(c)));
    // (the split down-projection and the token-reduction GEMM work on whole groups of 64 adapter rows)
    if (c.r < 0 || (c.r % 64) != 0 || c.r > 128) return set_error(FTMI_ERR_UNSUPPORTED, "wan_lora_ffn_block: LoRA rank must be 0, 64 or 128 (pad other ranks with zeros)");
    if (c.r > 0 && c.D < 256) return set_error(FTMI_ERR_UNSUPPORTED, "wan_lora_ffn_block: adapters need a width of at least 256");
    if (c.TI < 0 || c.TI > 320) return set_error(FTMI_ERR_UNSUPPORTED, "wan_lora_ffn_block: the image context holds 0 .. 320 tokens");
    if (c.TI2 < 0 || c.TI2 > 320) return set_error(FTMI_ERR_UNSUPPORTED, "wan_lora_ffn_block: a second image holds 0 .. 320 tokens");
    if (c.TI2 > 0 && c.TI == 0) return set_error(FTMI_ERR_INVALID, "wan_lora_ffn_block: a second image (TI2) needs a first one (TI > 0)");
    if (c.ffn != 0 && c.ffn != 1) return set_error(FTMI_ERR_INVALID, "wan_lora_ffn_block: ffn is 0 or 1");
    if (c.ffn && c.r == 0) return set_error(FTMI_ERR_UNSUPPORTED, "wan_lora_ffn_block: feed-forward adapters take the block's rank, which is 0");
    // (the split down-projection contracts over at least 256 columns: XA_2 = s act A_2^T and dXA_1 = s dpre B_1 contract over F)
    if (c.ffn && c.F < 256) return set_error(FTMI_ERR_UNSUPPORTED, "wan_lora_ffn_block: feed-forward adapters need a feed-forward width of at least 256");
    return 0;
}

// the frozen base's plan of one LoRA configuration (the byte planners pass no bases)
Bufs lora_layout(const ftmi_wan_lora_ffn_block_config& c, void* saved = nullptr, void* scratch = nullptr) {
    return make_layout(base_cfg(c), c.r, true, saved, scratch, c.TI + c.TI2, c.ffn != 0);  // the second image's rows follow the first one's
}

// the image context of attn2: TI tokens enc_img [B, TI, D] and the frozen flat buffer  add_k | add_v weight [2D, D], their biases [2D], norm_added_k [D]
struct ImgCtx {
    int TI = 0;         // all image tokens of a sample: both images of a first/last-frame model
    bool wide = false;  // a second image: the wide second-context kernels (attn_ctx2w_*), whatever the token count
    const bf16_t* params = nullptr;
    const bf16_t* enc = nullptr;
};

// the operand copies of one call's adapters and where its (hi | lo | hi) down-projections go
struct LoraOps {
    int r = 0;
    float s = 0.f;
    const bf16_t* sp = nullptr;   // forward: A as (hi, lo) row planes [8][2r][D];   backward: B^T planes [8][2r][D]
    const bf16_t* ext = nullptr;  // forward: B as [hi | hi | lo] columns [8][D][3r];   backward: A^T columns, the eight adapters side by side [D][24r]
    long ext_step = 0, ld_ext = 0;  // elements from one adapter's ext to the next, row stride of ext: forward 3 r D, 3r;   backward 3r, 24r
};

// `n` adjacent adapters on one projection, as one direction of the walk sees them (n = 0: a projection without adapters)
struct Adp {
    int n = 0, r = 0;
    float s = 0.f;
    const bf16_t* sp = nullptr;   // forward: A (hi, lo) row planes [n 2r, K_in];             backward: B^T planes [n 2r, N_out]
    const bf16_t* ext = nullptr;  // forward: B [hi | hi | lo] columns [n N_out, 3r];         backward: A^T columns [K_in, ld_ext], the n adapters side by side
    long ld_ext = 0;              // backward only
    bf16_t* xa = nullptr;         // [rows, 3 n r]: written by the forward, read by the backward
    float *ga = nullptr, *gb = nullptr;  // backward: fp32 [n r, K_in] / [n N_out, r] (ADDED to)
};

// K-contiguous copies of the weights for the input-gradient GEMMs (dX = dY W as an NT GEMM against W^T)
struct Twins {
    const bf16_t *qkv1 = nullptr, *o1 = nullptr, *q2 = nullptr, *kv2 = nullptr, *o2 = nullptr, *f1 = nullptr, *f2 = nullptr;
};

// What one call hands the walks.  Full fine-tune: lo.r = 0, grads and dmod set, twins transposed into scratch by the call.  Frozen base: grads = dmod = null,
// the caller's twins, the adapters' gradients in grad_a / grad_b when lo.r > 0.
struct Block {
    ftmi_wan_block_config c;
    const bf16_t* params = nullptr;
    Bufs L;
    LoraOps lo;
    const bf16_t *x = nullptr, *enc = nullptr;
    const float *mod = nullptr, *rope_cos = nullptr, *rope_sin = nullptr;
    float *grads = nullptr, *dmod = nullptr;      // backward: flat fp32 base gradients, fp32 [6, B, D] modulation sums (both ADDED to)
    float *grad_a = nullptr, *grad_b = nullptr;  // backward: fp32 [8, r, D] / [8, D, r] (ADDED to)
    Adp f1, f2;                                  // the feed-forward adapters on ffn.net.0.proj / ffn.net.2 (n = 0: none), filled for the call's direction
    Twins t;
    ImgCtx img;
    hipStream_t st = nullptr;
};

// dW += dY^T X (fp32), db += column sums of dY; nothing when the base is frozen (gw == null)
int linear_grads(const bf16_t* dy, long lddy, const bf16_t* inp, long ldi, int M, int N, int K, float* gw, float* gb, hipStream_t st) {
    if (!gw) return 0;
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
// q, k, o: token rows [B S, D]; v: the last D columns of the fused projection v_base [B Sk, ld_v]
AttnArgs attn_args(const ftmi_wan_block_config& c, const bf16_t* q, const bf16_t* k, const bf16_t* v_base, long ld_v, bf16_t* o, float* lse, int Sq, int Sk) {
    AttnArgs a;
    a.B = c.B; a.H = c.H; a.Sq = Sq; a.Sk = Sk; a.d = 128;
    a.scale = 0.08838834764831845f;  // 1 / sqrt(128)
    a.q = q; tok_strides(a.q_sb, a.q_sh, a.q_ss, Sq, c.D, 128);
    a.k = k; tok_strides(a.k_sb, a.k_sh, a.k_ss, Sk, c.D, 128);
    a.v = v_base + (ld_v - c.D); tok_strides(a.v_sb, a.v_sh, a.v_ss, Sk, ld_v, 128);
    a.o = o; tok_strides(a.o_sb, a.o_sh, a.o_ss, Sq, c.D, 128);
    a.lse2 = lse;
    return a;
}
// the backward's fields on top: dv goes where v sits in its fused projection, into dv_base
AttnArgs attn_bwd_args(AttnArgs a, const bf16_t* dout, bf16_t* dq, bf16_t* dk, bf16_t* dv_base, float* delta) {
    const long D = a.q_ss, ld_v = a.v_ss;
    a.dout = dout; tok_strides(a.do_sb, a.do_sh, a.do_ss, a.Sq, D, 128);
    a.dq = dq; tok_strides(a.dq_sb, a.dq_sh, a.dq_ss, a.Sq, D, 128);
    a.dk = dk; tok_strides(a.dk_sb, a.dk_sh, a.dk_ss, a.Sk, D, 128);
    a.dv = dv_base + (ld_v - D); tok_strides(a.dv_sb, a.dv_sh, a.dv_ss, a.Sk, ld_v, 128);
    a.delta = delta;
    return a;
}

// the attention adapters adp .. adp + nadp - 1 (order of the header comment) for the direction the call's LoraOps were filled for
Adp attn_adp(const Block& k, int adp, int nadp, bf16_t* xa) {
    Adp a;
    if (k.lo.r <= 0 || nadp <= 0) return a;
    const size_t r = k.lo.r, D = k.c.D;
    a.n = nadp; a.r = k.lo.r; a.s = k.lo.s; a.xa = xa;
    a.sp = k.lo.sp + adp * 2 * r * D;
    a.ext = k.lo.ext + adp * k.lo.ext_step;
    a.ld_ext = k.lo.ld_ext;
    if (k.grad_a) { a.ga = k.grad_a + adp * r * D; a.gb = k.grad_b + adp * D * r; }
    return a;
}

// s * X A^T (or s * dY B) of the adapters `ad` as ONE split down-projection contracting over K: out [rows, 3 n r]
int lora_down(const Adp& ad, const bf16_t* X, long ldx, int rows, int K, long xk_stride, bf16_t* out, hipStream_t st) {
    return gemm_nt(lora_down_args(X, ldx, rows, ad.sp, ad.n, K, ad.r, ad.s, out, xk_stride), st);
}

// out [rows, N] = X W^T + bias, X [rows, K], + the adapters `ad` on the same input (then N = ad.n N_out); ad.xa [rows, 3 n r] is kept for the backward.
// pre != null: out = gelu_tanh(the sum), pre = the sum (the feed-forward's first projection)
int proj_fwd(const Block& k, const bf16_t* X, int rows, int K, const bf16_t* Wm, const bf16_t* bias, int N, const Adp& ad, bf16_t* out, bf16_t* pre = nullptr) {
    GemmNtArgs a = linear_args(X, K, rows, Wm, K, N, K, bias, out, N, k.c.gemm_variant);
    if (pre) { a.out2 = pre; a.ldo2 = N; a.epi = EPI_GELU; }
    if (ad.n > 0) {
        FTMI_TRY(lora_down(ad, X, K, rows, K, 0, ad.xa, k.st));
        lora_ext_fwd(a, ad.xa, ad.n, ad.r, ad.ext);
    }
    return gemm_nt(a, k.st);
}

// The backward of proj_fwd for dY [rows, N], X [rows, K], Wt [K, N] the K-contiguous twin of W, in this order: dW += dY^T X and db += column sums (gw != null:
// the base trains); dXA = s dY B (adapters); dx [rows, K] = dY Wt^T (+ dXA A) (dx == null: skipped); dB += dY^T XA, dA += dXA^T X (adapters).
// pre != null: dx = (the sum) * gelu_tanh'(pre), pre [rows, K] (the feed-forward's second projection hands its input gradient through the activation)
int proj_bwd(const Block& k, const bf16_t* X, const bf16_t* dy, int rows, int N, int K, const bf16_t* Wt, const Adp& ad, bf16_t* dx, float* gw, float* gb,
             const bf16_t* pre = nullptr) {
    const int r = ad.n > 0 ? ad.r : 0, No = ad.n > 0 ? N / ad.n : N;  // (No: outputs per adapter)
    bf16_t* dxa = k.L.dxa;
    FTMI_TRY(linear_grads(dy, N, X, K, rows, N, K, gw, gb, k.st));
    if (r > 0) FTMI_TRY(lora_down(ad, dy, N, rows, No, ad.n > 1 ? No : 0, dxa, k.st));
    if (dx) {
        GemmNtArgs a = linear_args(dy, N, rows, Wt, N, K, N, nullptr, dx, K, k.c.gemm_variant);
        if (pre) { a.epi = EPI_DGELU; a.aux = pre; a.ldaux = K; }
        if (r > 0) lora_ext_bwd(a, dxa, ad.n, r, ad.ext, ad.ld_ext);
        FTMI_TRY(gemm_nt(a, k.st));
    }
    if (r > 0) {
        FTMI_TRY(gemm_tn(lora_db_args(dy, N, ad.xa, ad.n, r, No, ad.gb, rows), k.st));
        FTMI_TRY(gemm_tn(lora_da_args(dxa, ad.n, r, X, K, K, ad.ga, rows), k.st));
    }
    return 0;
}

// out == nullptr: the recomputation pass of gradient checkpointing -- the identical kernel sequence refills `saved` from the block's input and stops after
// the feed-forward's first GEMM (its pre-activation is the last thing the backward reads; with an adapter on ffn.net.2, its down-projected rows are)
int block_forward(const Block& k, bf16_t* out) {
    const ftmi_wan_block_config& c = k.c;
    const Bufs& L = k.L;
    const Offsets O = offsets_of(c.D, c.F);
    const int B = c.B, S = c.S, T = c.T, D = c.D, F = c.F, M = B * S, Mt = B * T;
    const float eps = c.eps;
    const long mb = 6L * D;  // sample stride of the modulation rows
    hipStream_t st = k.st;
    auto P = [&](size_t off) { return k.params + off; };
    auto MOD = [&](int i) { return k.mod + (size_t)i * D; };
    // self-attention
    {
        WanRowArgs a = row_args(k.x, D, L.n1, D, M, D, S, eps);
        a.shift = MOD(0); a.scale = MOD(1); a.mod_bstride = mb;
        FTMI_TRY(wan_ln_fwd(a, st));
    }
    FTMI_TRY(proj_fwd(k, L.n1, M, D, P(O.w_qkv1), P(O.b_qkv1), 3 * D, attn_adp(k, 0, 3, L.xa_qkv), L.qkv));
    for (int i = 0; i < 2; ++i) {
        WanRowArgs a = row_args(L.qkv + (size_t)i * D, 3 * D, i ? L.kn : L.qn, D, M, D, S, eps);
        a.w = P(i ? O.nk1 : O.nq1); a.rope_cos = k.rope_cos; a.rope_sin = k.rope_sin; a.head_dim = 128;
        FTMI_TRY(wan_rms_rope_fwd(a, st));
    }
    FTMI_TRY(attn_fwd(attn_args(c, L.qn, L.kn, L.qkv, 3 * D, L.o1, L.lse1, S, S), st));
    FTMI_TRY(proj_fwd(k, L.o1, M, D, P(O.w_o1), P(O.b_o1), D, attn_adp(k, 3, 1, L.xa_o1), L.a1));
    {
        WanRowArgs a = row_args(k.x, D, L.x1, D, M, D, S, eps);
        a.scale = MOD(2); a.mod_bstride = mb; a.dy = L.a1; a.ld_dy = D;
        FTMI_TRY(wan_gate_res_fwd(a, st));
    }
    // cross-attention to the text tokens (no rotary embedding, no gate)
    {
        WanRowArgs a = row_args(L.x1, D, L.n2, D, M, D, S, eps);
        a.w = P(O.n2w); a.b = P(O.n2b);
        FTMI_TRY(wan_ln_fwd(a, st));
    }
    FTMI_TRY(proj_fwd(k, L.n2, M, D, P(O.w_q2), P(O.b_q2), D, attn_adp(k, 4, 1, L.xa_q2), L.q2));
    FTMI_TRY(proj_fwd(k, k.enc, Mt, D, P(O.w_kv2), P(O.b_kv2), 2 * D, attn_adp(k, 5, 2, L.xa_kv2), L.kv2));
    {
        WanRowArgs a = row_args(L.q2, D, L.q2n, D, M, D, S, eps);
        a.w = P(O.nq2);
        FTMI_TRY(wan_rms_rope_fwd(a, st));
        WanRowArgs b = row_args(L.kv2, 2 * D, L.k2n, D, Mt, D, T, eps);
        b.w = P(O.nk2);
        FTMI_TRY(wan_rms_rope_fwd(b, st));
    }
    FTMI_TRY(attn_fwd(attn_args(c, L.q2n, L.k2n, L.kv2, 2 * D, L.o2, L.lse2, S, T), st));
    const bf16_t* o2 = L.o2;
    if (k.img.TI > 0) {  // the image tokens' keys and values (frozen, no adapters), then their attention summed onto the text branch's output
        const int TI = k.img.TI, Mi = B * TI;
        const bf16_t* ip = k.img.params;
        FTMI_TRY(proj_fwd(k, k.img.enc, Mi, D, ip, ip + 2 * (size_t)D * D, 2 * D, Adp(), L.kvi));
        WanRowArgs a = row_args(L.kvi, 2 * D, L.kin, D, Mi, D, TI, eps);
        a.w = ip + 2 * (size_t)D * D + 2 * D;
        FTMI_TRY(wan_rms_rope_fwd(a, st));
        FTMI_TRY((k.img.wide ? attn_ctx2w_fwd : attn_ctx2_fwd)(attn_args(c, L.q2n, L.kin, L.kvi, 2 * D, L.o2s, L.lse_i, S, TI), L.o2, st));
        o2 = L.o2s;
    }
    bf16_t* a2 = L.f;  // (the feed-forward output buffer doubles as the staging of o2 W_o2^T + b: it is consumed by the next launch)
    FTMI_TRY(proj_fwd(k, o2, M, D, P(O.w_o2), P(O.b_o2), D, attn_adp(k, 7, 1, L.xa_o2), a2));
    {
        WanRowArgs a = row_args(L.x1, D, L.x2, D, M, D, S, eps);
        a.dy = a2; a.ld_dy = D;
        FTMI_TRY(wan_gate_res_fwd(a, st));
    }
    // feed-forward
    {
        WanRowArgs a = row_args(L.x2, D, L.n3, D, M, D, S, eps);
        a.shift = MOD(3); a.scale = MOD(4); a.mod_bstride = mb;
        FTMI_TRY(wan_ln_fwd(a, st));
    }
    FTMI_TRY(proj_fwd(k, L.n3, M, D, P(O.w_f1), P(O.b_f1), F, k.f1, L.act, L.pre));  // GELU-tanh, pre-activation kept
    if (!out) return k.f2.n > 0 ? lora_down(k.f2, L.act, F, M, F, 0, k.f2.xa, st) : 0;
    FTMI_TRY(proj_fwd(k, L.act, M, F, P(O.w_f2), P(O.b_f2), D, k.f2, L.f));
    {
        WanRowArgs a = row_args(L.x2, D, out, D, M, D, S, eps);
        a.scale = MOD(5); a.mod_bstride = mb; a.dy = L.f; a.ld_dy = D;
        FTMI_TRY(wan_gate_res_fwd(a, st));
    }
    return 0;
}

// dx [B, S, D] written; denc [B, T, D] written, or null (frozen text embedder: its GEMM is skipped).  A frozen base (k.grads == k.dmod == null) turns every
// base-gradient launch and every row-wise reduction off through the null pointers G and DMOD return.
int block_backward(const Block& k, const bf16_t* dout, bf16_t* dx, bf16_t* denc) {
    const ftmi_wan_block_config& c = k.c;
    const Bufs& L = k.L;
    const Offsets O = offsets_of(c.D, c.F);
    const int B = c.B, S = c.S, T = c.T, D = c.D, F = c.F, M = B * S, Mt = B * T;
    const float eps = c.eps;
    const long mb = 6L * D;
    hipStream_t st = k.st;
    auto P = [&](size_t off) { return k.params + off; };
    auto G = [&](size_t off) { return k.grads ? k.grads + off : nullptr; };
    auto MOD = [&](int i) { return k.mod + (size_t)i * D; };
    auto DMOD = [&](int i) { return k.dmod ? k.dmod + (size_t)i * B * D : nullptr; };
    const int per_batch = k.dmod != nullptr;
    // y = d out * gate;  d gate += sum d out * branch when the gate trains (the only reader of the branch output)
    auto gate_bwd = [&](const bf16_t* d_out, bf16_t* y, const bf16_t* branch, int gate) {
        WanRowArgs a = row_args(d_out, D, y, D, M, D, S, eps);
        a.scale = MOD(gate); a.mod_bstride = mb; a.red1 = DMOD(gate); a.red_per_batch = per_batch;
        if (a.red1) { a.dy = branch; a.ld_dy = D; }
        return wan_gate_res_bwd(a, st);
    };

    // feed-forward branch: out = x2 + f * gate_ff
    FTMI_TRY(gate_bwd(dout, L.df, L.f, 5));
    FTMI_TRY(proj_bwd(k, L.act, L.df, M, D, F, k.t.f2, k.f2, L.dpre, G(O.w_f2), G(O.b_f2), L.pre));  // (d f W2 [+ dXA_2 A_2]) * gelu'(pre)
    FTMI_TRY(proj_bwd(k, L.n3, L.dpre, M, F, D, k.t.f1, k.f1, L.dn3, G(O.w_f1), G(O.b_f1)));
    {
        WanRowArgs a = row_args(L.x2, D, L.dx2, D, M, D, S, eps);
        a.scale = MOD(4); a.mod_bstride = mb; a.dy = L.dn3; a.ld_dy = D; a.dres = dout; a.red1 = DMOD(3); a.red2 = DMOD(4); a.red_per_batch = per_batch;
        FTMI_TRY(wan_ln_bwd(a, st));
    }
    // cross-attention branch: x2 = x1 + a2
    FTMI_TRY(proj_bwd(k, k.img.TI > 0 ? L.o2s : L.o2, L.dx2, M, D, D, k.t.o2, attn_adp(k, 7, 1, L.xa_o2), L.do2, G(O.w_o2), G(O.b_o2)));
    FTMI_TRY(attn_bwd(attn_bwd_args(attn_args(c, L.q2n, L.k2n, L.kv2, 2 * D, L.o2, L.lse2, S, T), L.do2, L.dq2n, L.dk2n, L.dkv2, L.delta), st));
    if (k.img.TI > 0)  // the image branch's dQ, added onto the text branch's in place (its keys and values are frozen: no dK, dV)
        FTMI_TRY((k.img.wide ? attn_ctx2w_dq : attn_ctx2_dq)(attn_bwd_args(attn_args(c, L.q2n, L.kin, L.kvi, 2 * D, L.o2s, L.lse_i, S, k.img.TI), L.do2, L.dq2n, nullptr, L.dkv2, nullptr), L.dq2n, st));
    {
        WanRowArgs a = row_args(L.q2, D, L.dq2, D, M, D, S, eps);
        a.w = P(O.nq2); a.dy = L.dq2n; a.ld_dy = D; a.red2 = G(O.nq2);
        FTMI_TRY(wan_rms_rope_bwd(a, st));
        WanRowArgs b = row_args(L.kv2, 2 * D, L.dkv2, 2 * D, Mt, D, T, eps);
        b.w = P(O.nk2); b.dy = L.dk2n; b.ld_dy = D; b.red2 = G(O.nk2);
        FTMI_TRY(wan_rms_rope_bwd(b, st));
    }
    FTMI_TRY(linear_grads(L.dq2, D, L.n2, D, M, D, D, G(O.w_q2), G(O.b_q2), st));  // (attn2.to_q's weight gradient goes ahead of the text rows' projection)
    FTMI_TRY(proj_bwd(k, k.enc, L.dkv2, Mt, 2 * D, D, k.t.kv2, attn_adp(k, 5, 2, L.xa_kv2), denc, G(O.w_kv2), G(O.b_kv2)));
    FTMI_TRY(proj_bwd(k, L.n2, L.dq2, M, D, D, k.t.q2, attn_adp(k, 4, 1, L.xa_q2), L.dn2, nullptr, nullptr));
    {
        WanRowArgs a = row_args(L.x1, D, L.dx1, D, M, D, S, eps);
        a.w = P(O.n2w); a.dy = L.dn2; a.ld_dy = D; a.dres = L.dx2; a.red1 = G(O.n2b); a.red2 = G(O.n2w);
        FTMI_TRY(wan_ln_bwd(a, st));
    }
    // self-attention branch: x1 = x + a1 * gate_msa
    FTMI_TRY(gate_bwd(L.dx1, L.da1, L.a1, 2));
    FTMI_TRY(proj_bwd(k, L.o1, L.da1, M, D, D, k.t.o1, attn_adp(k, 3, 1, L.xa_o1), L.do1, G(O.w_o1), G(O.b_o1)));
    FTMI_TRY(attn_bwd(attn_bwd_args(attn_args(c, L.qn, L.kn, L.qkv, 3 * D, L.o1, L.lse1, S, S), L.do1, L.dqn, L.dkn, L.dqkv, L.delta), st));
    for (int i = 0; i < 2; ++i) {
        WanRowArgs a = row_args(L.qkv + (size_t)i * D, 3 * D, L.dqkv + (size_t)i * D, 3 * D, M, D, S, eps);
        a.w = P(i ? O.nk1 : O.nq1); a.dy = i ? L.dkn : L.dqn; a.ld_dy = D; a.red2 = G(i ? O.nk1 : O.nq1); a.rope_cos = k.rope_cos; a.rope_sin = k.rope_sin; a.head_dim = 128;
        FTMI_TRY(wan_rms_rope_bwd(a, st));
    }
    // the three projections' input gradients (and their adapters') summed in the fp32 accumulator
    FTMI_TRY(proj_bwd(k, L.n1, L.dqkv, M, 3 * D, D, k.t.qkv1, attn_adp(k, 0, 3, L.xa_qkv), L.dn1, G(O.w_qkv1), G(O.b_qkv1)));
    {
        WanRowArgs a = row_args(k.x, D, dx, D, M, D, S, eps);
        a.scale = MOD(1); a.mod_bstride = mb; a.dy = L.dn1; a.ld_dy = D; a.dres = L.dx1; a.red1 = DMOD(0); a.red2 = DMOD(1); a.red_per_batch = per_batch;
        FTMI_TRY(wan_ln_bwd(a, st));
    }
    return 0;
}

Block make_block(const ftmi_wan_block_config& c, const void* params, const Bufs& L, const bf16_t* x, const bf16_t* enc, const float* mod, const float* rope_cos,
                 const float* rope_sin, hipStream_t st) {
    Block k;
    k.c = c; k.params = reinterpret_cast<const bf16_t*>(params); k.L = L; k.x = x; k.enc = enc; k.mod = mod; k.rope_cos = rope_cos; k.rope_sin = rope_sin; k.st = st;
    return k;
}

}  // namespace

size_t wan_block_saved_bytes(const ftmi_wan_block_config& c) { return make_layout(c, 0, false).saved_total; }
size_t wan_block_scratch_bytes(const ftmi_wan_block_config& c) { return make_layout(c, 0, false).scratch_total; }
size_t wan_block_param_elements(const ftmi_wan_block_config& c) { return offsets_of(c.D, c.F).total; }

int wan_block_forward(const ftmi_wan_block_config& c, const bf16_t* params, const bf16_t* x, const bf16_t* enc, const float* mod, const float* rope_cos,
                      const float* rope_sin, bf16_t* out, void* saved, size_t saved_bytes, hipStream_t st) {
    FTMI_TRY(check_cfg(c));
    const Bufs L = make_layout(c, 0, false, saved);
    if (saved_bytes < L.saved_total) return set_error(FTMI_ERR_INVALID, "wan_block_forward: saved buffer too small");
    return block_forward(make_block(c, params, L, x, enc, mod, rope_cos, rope_sin, st), out);
}

// grads: the block's flat fp32 gradient buffer (ADDED to); dmod fp32 [6, B, D] (ADDED to: column sums of d shift / d scale / d gate per sample);
// dx [B, S, D], denc [B, T, D] written.
int wan_block_backward(const ftmi_wan_block_config& c, const bf16_t* params, float* grads, const bf16_t* x, const bf16_t* enc, const float* mod,
                       const float* rope_cos, const float* rope_sin, const bf16_t* dout, bf16_t* dx, bf16_t* denc, float* dmod, void* saved,
                       size_t saved_bytes, void* scratch, size_t scratch_bytes, hipStream_t st) {
    FTMI_TRY(check_cfg(c));
    const Bufs L = make_layout(c, 0, false, saved, scratch);
    if (saved_bytes < L.saved_total || scratch_bytes < L.scratch_total) return set_error(FTMI_ERR_INVALID, "wan_block_backward: buffer too small");
    Block k = make_block(c, params, L, x, enc, mod, rope_cos, rope_sin, st);
    k.grads = grads; k.dmod = dmod;
    const Offsets O = offsets_of(c.D, c.F);
    const int D = c.D, F = c.F;
    // the weights train: their K-contiguous copies are made per call
    FTMI_TRY(transpose_bf16(params + O.w_f2, L.t_f2, D, F, st));
    FTMI_TRY(transpose_bf16(params + O.w_f1, L.t_f1, F, D, st));
    FTMI_TRY(transpose_bf16(params + O.w_o2, L.t_o2, D, D, st));
    FTMI_TRY(transpose_bf16(params + O.w_q2, L.t_q2, D, D, st));
    FTMI_TRY(transpose_bf16(params + O.w_kv2, L.t_kv2, 2 * D, D, st));
    FTMI_TRY(transpose_bf16(params + O.w_o1, L.t_o1, D, D, st));
    FTMI_TRY(transpose_bf16(params + O.w_qkv1, L.t_qkv1, 3 * D, D, st));
    k.t.qkv1 = L.t_qkv1; k.t.o1 = L.t_o1; k.t.q2 = L.t_q2; k.t.kv2 = L.t_kv2; k.t.o2 = L.t_o2; k.t.f1 = L.t_f1; k.t.f2 = L.t_f2;
    return block_backward(k, dout, dx, denc);
}

namespace {

// one fp32 matrix [rows, cols] into one of its four operand layouts (LoraSplitArgs)
int split_one(const float* wm, int rows, int cols, bf16_t* sp, bf16_t* ext, bf16_t* t_sp, bf16_t* t_ext, hipStream_t st) {
    LoraSplitArgs a;
    a.w = wm; a.rows = rows; a.cols = cols; a.nmat = 1; a.sp = sp; a.ext = ext; a.ld_ext = 3L * cols; a.t_sp = t_sp; a.t_ext = t_ext; a.ld_t_ext = 3L * rows;
    return lora_split(a, st);
}

Adp ffn_adp(const ftmi_wan_lora_ffn_block_config& c, const bf16_t* sp, const bf16_t* ext, bf16_t* xa, float* ga, float* gb) {
    Adp a;
    a.n = 1; a.r = c.r; a.s = c.lora_scale; a.sp = sp; a.ext = ext; a.ld_ext = 3L * c.r; a.xa = xa; a.ga = ga; a.gb = gb;
    return a;
}

// the frozen-base block of one LoRA call: its plan, its parameters and the image context of attn2 (TI = 0: none)
Block lora_block(const ftmi_wan_lora_ffn_block_config& c, const ftmi_wan_lora_ffn_block_weights& w, const Bufs& L, const bf16_t* img_params, const bf16_t* x,
                 const bf16_t* enc, const bf16_t* enc_img, const float* mod, const float* rope_cos, const float* rope_sin, hipStream_t st) {
    Block k = make_block(base_cfg(c), w.base.params, L, x, enc, mod, rope_cos, rope_sin, st);
    k.img.TI = c.TI + c.TI2; k.img.wide = c.TI2 > 0; k.img.params = img_params; k.img.enc = enc_img;
    k.lo.r = c.r; k.lo.s = c.lora_scale;
    return k;
}

}  // namespace

// The LoRA block: adapters on the eight attention projections (cfg.r, 0: none), the image context of attn2 (cfg.TI image tokens, 0: none: text-to-video) and,
// cfg.ffn = 1, adapters on the two feed-forward projections as well.  (The planners return 0 for a configuration the block refuses: the message is in
// ftmi_last_error.)
size_t wan_lora_ffn_block_saved_bytes(const ftmi_wan_lora_ffn_block_config& c) { return check_lora_cfg(c) ? 0 : lora_layout(c).saved_total; }
size_t wan_lora_ffn_block_scratch_bytes(const ftmi_wan_lora_ffn_block_config& c) { return check_lora_cfg(c) ? 0 : lora_layout(c).scratch_total; }

int wan_lora_ffn_block_forward(const ftmi_wan_lora_ffn_block_config& c, const ftmi_wan_lora_ffn_block_weights& w, const bf16_t* img_params, const bf16_t* x,
                               const bf16_t* enc, const bf16_t* enc_img, const float* mod, const float* rope_cos, const float* rope_sin, bf16_t* out, void* saved,
                               size_t saved_bytes, void* scratch, size_t scratch_bytes, hipStream_t st) {
    FTMI_TRY(check_lora_cfg(c));
    if (c.TI > 0 && (!img_params || !enc_img)) return set_error(FTMI_ERR_INVALID, "wan_lora_ffn_block_forward: image tokens without their parameters");
    if (c.ffn && (!w.ffn_a1 || !w.ffn_b1 || !w.ffn_a2 || !w.ffn_b2)) return set_error(FTMI_ERR_INVALID, "wan_lora_ffn_block_forward: feed-forward adapters missing");
    const Bufs L = lora_layout(c, saved, scratch);
    if (saved_bytes < L.saved_total || scratch_bytes < L.scratch_total) return set_error(FTMI_ERR_INVALID, "wan_lora_ffn_block_forward: buffer too small");
    if (c.r > 0 && (!w.base.lora_a || !w.base.lora_b)) return set_error(FTMI_ERR_INVALID, "wan_lora_ffn_block_forward: LoRA rank without adapters");
    Block k = lora_block(c, w, L, img_params, x, enc, enc_img, mod, rope_cos, rope_sin, st);
    const int D = c.D, F = c.F, r = c.r;
    if (r > 0) {  // operand copies of the fp32 adapters, once per call: A as (hi, lo) row planes, B as [hi | hi | lo] K-extension columns
        LoraSplitArgs sa;
        sa.w = w.base.lora_a; sa.rows = r; sa.cols = D; sa.nmat = 8; sa.in_bstride = (long)r * D; sa.sp = L.a_sp; sa.sp_bstride = 2L * r * D;
        FTMI_TRY(lora_split(sa, st));
        LoraSplitArgs sb;
        sb.w = w.base.lora_b; sb.rows = D; sb.cols = r; sb.nmat = 8; sb.in_bstride = (long)D * r; sb.ext = L.b_ext; sb.ext_bstride = 3L * D * r; sb.ld_ext = 3 * r;
        FTMI_TRY(lora_split(sb, st));
        k.lo.sp = L.a_sp; k.lo.ext = L.b_ext; k.lo.ext_step = 3L * r * D; k.lo.ld_ext = 3L * r;
    }
    if (c.ffn) {
        FTMI_TRY(split_one(w.ffn_a1, r, D, L.f_a1_sp, nullptr, nullptr, nullptr, st));
        FTMI_TRY(split_one(w.ffn_b1, F, r, nullptr, L.f_b1_ext, nullptr, nullptr, st));
        FTMI_TRY(split_one(w.ffn_a2, r, F, L.f_a2_sp, nullptr, nullptr, nullptr, st));
        FTMI_TRY(split_one(w.ffn_b2, D, r, nullptr, L.f_b2_ext, nullptr, nullptr, st));
        k.f1 = ffn_adp(c, L.f_a1_sp, L.f_b1_ext, L.xa_f1, nullptr, nullptr);
        k.f2 = ffn_adp(c, L.f_a2_sp, L.f_b2_ext, L.xa_f2, nullptr, nullptr);
    }
    return block_forward(k, out);
}

// grad_a fp32 [8, r, D] / grad_b fp32 [8, D, r] and the feed-forward adapters' grad_ffn_a1 [r, D], grad_ffn_b1 [F, r], grad_ffn_a2 [r, F], grad_ffn_b2 [D, r] ADDED to.
int wan_lora_ffn_block_backward(const ftmi_wan_lora_ffn_block_config& c, const ftmi_wan_lora_ffn_block_weights& w, const bf16_t* img_params, const bf16_t* x,
                                const bf16_t* enc, const bf16_t* enc_img, const float* mod, const float* rope_cos, const float* rope_sin, const bf16_t* dout,
                                bf16_t* dx, bf16_t* denc, float* grad_a, float* grad_b, float* grad_ffn_a1, float* grad_ffn_b1, float* grad_ffn_a2,
                                float* grad_ffn_b2, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, hipStream_t st) {
    FTMI_TRY(check_lora_cfg(c));
    if (c.TI > 0 && (!img_params || !enc_img)) return set_error(FTMI_ERR_INVALID, "wan_lora_ffn_block_backward: image tokens without their parameters");
    if (c.ffn && (!w.ffn_a1 || !w.ffn_b1 || !w.ffn_a2 || !w.ffn_b2 || !grad_ffn_a1 || !grad_ffn_b1 || !grad_ffn_a2 || !grad_ffn_b2))
        return set_error(FTMI_ERR_INVALID, "wan_lora_ffn_block_backward: feed-forward adapters / gradient buffers missing");
    const ftmi_wan_lora_block_weights& wb = w.base;
    const Bufs L = lora_layout(c, saved, scratch);
    if (saved_bytes < L.saved_total || scratch_bytes < L.scratch_total) return set_error(FTMI_ERR_INVALID, "wan_lora_ffn_block_backward: buffer too small");
    if (c.r > 0 && (!wb.lora_a || !wb.lora_b || !grad_a || !grad_b))
        return set_error(FTMI_ERR_INVALID, "wan_lora_ffn_block_backward: LoRA rank without adapters / gradient buffers");
    if (!wb.w_qkv1_t || !wb.w_o1_t || !wb.w_q2_t || !wb.w_kv2_t || !wb.w_o2_t || !wb.w_f1_t || !wb.w_f2_t)
        return set_error(FTMI_ERR_INVALID, "wan_lora_ffn_block_backward: transposed weights missing");
    Block k = lora_block(c, w, L, img_params, x, enc, enc_img, mod, rope_cos, rope_sin, st);
    auto WT = [](const void* p) { return reinterpret_cast<const bf16_t*>(p); };
    k.t.qkv1 = WT(wb.w_qkv1_t); k.t.o1 = WT(wb.w_o1_t); k.t.q2 = WT(wb.w_q2_t); k.t.kv2 = WT(wb.w_kv2_t); k.t.o2 = WT(wb.w_o2_t); k.t.f1 = WT(wb.w_f1_t); k.t.f2 = WT(wb.w_f2_t);
    k.grad_a = grad_a; k.grad_b = grad_b;
    const int D = c.D, F = c.F, r = c.r;
    if (r > 0) {
        LoraSplitArgs sb;  // B^T as (hi, lo) row planes: operand of dXA = s * dY B
        sb.w = wb.lora_b; sb.rows = D; sb.cols = r; sb.nmat = 8; sb.in_bstride = (long)D * r; sb.t_sp = L.bt_sp; sb.t_sp_bstride = 2L * r * D;
        FTMI_TRY(lora_split(sb, st));
        LoraSplitArgs sa;  // A^T as K-extension columns, the eight adapters side by side [D, 24r]: dx += dXA A, fused projections take adjacent column groups
        sa.w = wb.lora_a; sa.rows = r; sa.cols = D; sa.nmat = 8; sa.in_bstride = (long)r * D; sa.t_ext = L.at_ext; sa.t_ext_bstride = 3L * r; sa.ld_t_ext = 24L * r;
        FTMI_TRY(lora_split(sa, st));
        k.lo.sp = L.bt_sp; k.lo.ext = L.at_ext; k.lo.ext_step = 3L * r; k.lo.ld_ext = 24L * r;
    }
    if (c.ffn) {  // B^T as (hi, lo) row planes, A^T as K-extension columns, per adapter
        FTMI_TRY(split_one(w.ffn_b1, F, r, nullptr, nullptr, L.f_b1t_sp, nullptr, st));
        FTMI_TRY(split_one(w.ffn_a1, r, D, nullptr, nullptr, nullptr, L.f_a1t_ext, st));
        FTMI_TRY(split_one(w.ffn_b2, D, r, nullptr, nullptr, L.f_b2t_sp, nullptr, st));
        FTMI_TRY(split_one(w.ffn_a2, r, F, nullptr, nullptr, nullptr, L.f_a2t_ext, st));
        k.f1 = ffn_adp(c, L.f_b1t_sp, L.f_a1t_ext, L.xa_f1, grad_ffn_a1, grad_ffn_b1);
        k.f2 = ffn_adp(c, L.f_b2t_sp, L.f_a2t_ext, L.xa_f2, grad_ffn_a2, grad_ffn_b2);
    }
    return block_backward(k, dout, dx, denc);
}

}  // namespace ftmi
