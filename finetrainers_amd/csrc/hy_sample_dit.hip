// HunyuanVideo latent sampling: the whole denoising loop of a validation run as ONE call (include/ftmi355.h: ftmi_hy_sample_text; the layout and step kernels
// are in sample_layout.hip, the two block orchestrators in hy_dit.hip).
// Restates what the reference gets from HunyuanVideoPipeline over the transformer it trains (finetrainers/models/hunyuan_video/base_specification.py:332-355),
// in latent space, text-to-video.  Per step, on one stream, no host synchronisation -- the launches of MI355XHunyuanVideoTransformer3DModel.forward (under
// no_grad) at batch P B, in its order, so the bits are its bits:
//   patch embedding                 ONE NT GEMM over all P B S rows of cols -> the video stream [P B, S, D]
//   Ld x hy_dual_forward            one call per sample row, as the module loops; the text rows of block 0 are the step's refined text; the two streams alternate
//                                   between two buffers each; the LAST dual block writes out_t / out_v straight into the rows of the joint buffer
//                                   [P B, T + S, D], text first (the model's torch.cat).  Ld = 0: the embedding and the step's text are copied there.
//   Ls x hy_single_forward          at batch P B, alternating between two joint buffers
//   output norm                     cog_ln_mod_fwd on the video rows of each sample row with its shift / 1 + scale of the step, no affine (_HeadFunction.forward)
//   proj_out                        NT GEMM -> pred [P B S, Kc]
//   hy_sample_step                  true-CFG combine + flow-match Euler update on the state, bf16 copies into cols
// fp8 storage: a block's bf16 weights exist only after its up-cast into the arena all blocks share, so the up-casts of the block's list are queued right
// before its launches, every block of every step (the order _materialize_fwd keeps).
// Workspace: two video and two text stream buffers, two joint buffers, ONE `saved` slot and ONE scratch area (each the larger of the dual and the single
// block's need), the head's normalised rows and pred.  Nothing in it grows with Ld or Ls.
#include "common.hip.h"
#include "kernels.h"
#include "lora_proj.hip.h"

namespace ftmi {

namespace {

struct HySamplePlan {
    size_t xv[2], xt[2], joint[2], saved, scratch, hn, pred, total;
    size_t saved_dual, saved_single, scratch_dual, scratch_single;
    long S, Kc;
    ftmi_hy_dual_config dc;
    ftmi_hy_single_config sc;
};

int make_plan(const ftmi_hy_sample_config& c, int text_adapters, HySamplePlan& p) {
    const ftmi_hy_sample_geometry& g = c.geo;
    if (g.B <= 0 || g.C <= 0 || g.F <= 0 || g.H <= 0 || g.W <= 0 || g.p <= 0 || g.pt <= 0 || c.T <= 0 || c.steps <= 0)
        return set_error(FTMI_ERR_INVALID, "hy_sample: extents and steps must be positive");
    if (c.Ld < 0 || c.Ls < 0 || c.Ld + c.Ls == 0) return set_error(FTMI_ERR_INVALID, "hy_sample: at least one block");
    if (g.F % g.pt || g.H % g.p || g.W % g.p) return set_error(FTMI_ERR_UNSUPPORTED, "hy_sample: the latent size must be whole patches");
    if ((c.true_cfg != 1.0f) != (g.P == 2) || (g.P != 1 && g.P != 2)) return set_error(FTMI_ERR_INVALID, "hy_sample: P is 2 with true_cfg != 1 and 1 with true_cfg == 1");
    p.S = (long)(g.F / g.pt) * (g.H / g.p) * (g.W / g.p);
    p.Kc = (long)g.C * g.pt * g.p * g.p;
    if (p.Kc % 64 || p.Kc > 2048) return set_error(FTMI_ERR_UNSUPPORTED, "hy_sample: C pt p p must be a multiple of 64 (GEMM), at most 2048");
    if ((long)g.P * g.B * (c.T + p.S) > 0x7fffffffL) return set_error(FTMI_ERR_UNSUPPORTED, "hy_sample: too many tokens");
    const int rows = g.P * g.B;
    ftmi_hy_dual_config& d = p.dc;
    d.T = c.T; d.S = (int)p.S; d.D = c.D; d.H = c.H; d.mlp = c.mlp; d.r = c.r; d.lora_scale = c.lora_scale; d.eps = c.eps; d.gemm_variant = c.gemm_variant;
    d.text_adapters = text_adapters;  // the dual blocks' lora_a / lora_b hold eight matrices; the single blocks have no text projections of their own
    ftmi_hy_single_config& s = p.sc;
    s.B = rows; s.T = c.T; s.S = (int)p.S; s.D = c.D; s.H = c.H; s.mlp = c.mlp; s.r = c.r; s.lora_scale = c.lora_scale; s.eps = c.eps; s.gemm_variant = c.gemm_variant;
    // the two block orchestrators refuse the same widths and ranks; asking the bytes of a refused configuration would size buffers from nonsense
    if (c.H * 128 != c.D || c.D % 128 != 0 || c.D > 4096) return set_error(FTMI_ERR_UNSUPPORTED, "hy_sample: width must be heads x 128, at most 4096");
    if (c.r < 0 || (c.r % 64) != 0) return set_error(FTMI_ERR_UNSUPPORTED, "hy_sample: LoRA rank must be 0 or a multiple of 64 (pad smaller ranks with zeros)");
    if (c.mlp <= 0 || (c.mlp % 128)) return set_error(FTMI_ERR_UNSUPPORTED, "hy_sample: the feed-forward width must be a multiple of 128");
    if ((text_adapters != 0 && text_adapters != 1) || (text_adapters == 1 && c.r == 0))
        return set_error(FTMI_ERR_INVALID, "hy_sample: text_adapters is 0 or 1, and 1 needs a LoRA rank");
    p.saved_dual = hy_dual_saved_bytes(d); p.scratch_dual = hy_dual_scratch_bytes(d);
    p.saved_single = hy_single_saved_bytes(s); p.scratch_single = hy_single_scratch_bytes(s);
    const size_t Mv = (size_t)rows * p.S, Mt = (size_t)rows * c.T, D = c.D, e2 = 2;
    Bump w;
    for (int i = 0; i < 2; ++i) p.xv[i] = w.take(Mv * D * e2);
    for (int i = 0; i < 2; ++i) p.xt[i] = w.take(Mt * D * e2);
    for (int i = 0; i < 2; ++i) p.joint[i] = w.take((Mv + Mt) * D * e2);
    p.saved = w.take(p.saved_dual > p.saved_single ? p.saved_dual : p.saved_single);
    p.scratch = w.take(p.scratch_dual > p.scratch_single ? p.scratch_dual : p.scratch_single);
    p.hn = w.take(Mv * D * e2);
    p.pred = w.take(Mv * p.Kc * e2);
    p.total = w.off;
    return 0;
}

int copy_rows(bf16_t* dst, const bf16_t* src, size_t elements, hipStream_t st) {
    if (hipMemcpyAsync(dst, src, elements * 2, hipMemcpyDeviceToDevice, st) != hipSuccess) return set_error(FTMI_ERR_LAUNCH, "hy_sample: copy into the joint buffer failed");
    return 0;
}

}  // namespace

size_t hy_sample_workspace_bytes(const ftmi_hy_sample_config& c, int text_adapters) {
    HySamplePlan p;
    return make_plan(c, text_adapters, p) ? 0 : p.total;
}

int hy_sample(const ftmi_hy_sample_config& c, int text_adapters, const ftmi_hy_sample_weights& w, bf16_t* cols, float* x, const bf16_t* temb_silu, const bf16_t* enc,
              const bf16_t* head_shift, const bf16_t* head_onep, const float* key_bias, const float* rope_cos, const float* rope_sin, const float* sigmas, void* ws,
              size_t ws_bytes, hipStream_t st) {
    HySamplePlan p;
    FTMI_TRY(make_plan(c, text_adapters, p));
    if (ws_bytes < p.total) return set_error(FTMI_ERR_INVALID, "hy_sample: workspace too small (ftmi_hy_sample_text_workspace_bytes)");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return set_error(FTMI_ERR_INVALID, "hy_sample: the workspace must be 256-byte aligned");
    if (!w.patch_w || !w.patch_b || !w.proj_w || !w.proj_b || !w.ones || !w.zeros || (c.Ld > 0 && !w.dual) || (c.Ls > 0 && !w.single))
        return set_error(FTMI_ERR_INVALID, "hy_sample: weights missing");
    if (w.upcasts && (!w.upcast_count || !w.arena)) return set_error(FTMI_ERR_INVALID, "hy_sample: the up-cast lists come with their counts and the arena");
    const ftmi_hy_sample_geometry& g = c.geo;
    const int D = c.D, T = c.T, S = (int)p.S, N = T + S, rows = g.P * g.B, Kc = (int)p.Kc, V = c.gemm_variant;
    bf16_t *xv[2] = {W(ws, p.xv[0]), W(ws, p.xv[1])}, *xt[2] = {W(ws, p.xt[0]), W(ws, p.xt[1])}, *joint[2] = {W(ws, p.joint[0]), W(ws, p.joint[1])};
    bf16_t *hn = W(ws, p.hn), *pred = W(ws, p.pred);
    void *saved = reinterpret_cast<char*>(ws) + p.saved, *scratch = reinterpret_cast<char*>(ws) + p.scratch;

    for (int i = 0; i < c.steps; ++i) {
        const bf16_t* temb_i = temb_silu + (size_t)i * rows * D;
        const bf16_t* enc_i = enc + (size_t)i * rows * T * D;
        const ftmi_hy_sample_upcast* up = w.upcasts;
        auto upcast_block = [&](int blk) -> int {  // fp8 storage: this block's bf16 weights into the shared arena, right before its launches
            if (!w.upcasts) return 0;
            for (int k = 0; k < w.upcast_count[blk]; ++k, ++up)
                FTMI_TRY(fp8_upcast(reinterpret_cast<const uint8_t*>(up->src), reinterpret_cast<bf16_t*>(w.arena) + up->offset, up->rows, up->cols, 0, st));
            return 0;
        };
        FTMI_TRY(gemm_nt(linear_args(cols, Kc, rows * S, P(w.patch_w, 0), Kc, D, Kc, P(w.patch_b, 0), xv[0], D, V), st));
        for (int l = 0; l < c.Ld; ++l) {
            FTMI_TRY(upcast_block(l));
            const bool last = l == c.Ld - 1;
            const bf16_t* tin = l == 0 ? enc_i : xt[l & 1];
            for (int m = 0; m < rows; ++m) {
                bf16_t* ov = last ? joint[0] + ((size_t)m * N + T) * D : xv[(l + 1) & 1] + (size_t)m * S * D;
                bf16_t* ot = last ? joint[0] + (size_t)m * N * D : xt[(l + 1) & 1] + (size_t)m * T * D;
                FTMI_TRY(hy_dual_forward(p.dc, w.dual[l], xv[l & 1] + (size_t)m * S * D, tin + (size_t)m * T * D, temb_i + (size_t)m * D,
                                         key_bias ? key_bias + (size_t)m * N : nullptr, rope_cos, rope_sin, ov, ot, saved, p.saved_dual, scratch, p.scratch_dual, st));
            }
        }
        if (c.Ld == 0)
            for (int m = 0; m < rows; ++m) {
                FTMI_TRY(copy_rows(joint[0] + (size_t)m * N * D, enc_i + (size_t)m * T * D, (size_t)T * D, st));
                FTMI_TRY(copy_rows(joint[0] + ((size_t)m * N + T) * D, xv[0] + (size_t)m * S * D, (size_t)S * D, st));
            }
        for (int l = 0; l < c.Ls; ++l) {
            FTMI_TRY(upcast_block(c.Ld + l));
            FTMI_TRY(hy_single_forward(p.sc, w.single[l], joint[l & 1], temb_i, key_bias, rope_cos, rope_sin, joint[(l + 1) & 1], saved, p.saved_single, scratch,
                                       p.scratch_single, st));
        }
        const bf16_t* out = joint[c.Ls & 1];
        for (int m = 0; m < rows; ++m) {  // the output norm on the video rows of a sample row (contiguous; the sample rows are T rows apart)
            CogLnArgs a;
            a.x = out + ((size_t)m * N + T) * D; a.w = P(w.ones, 0); a.b = P(w.zeros, 0); a.shift = head_shift + ((size_t)i * rows + m) * D;
            a.onep = head_onep + ((size_t)i * rows + m) * D; a.y = hn + (size_t)m * S * D; a.rows = S; a.D = D; a.rows_per_batch = S; a.seg0 = 0; a.eps = c.eps;
            FTMI_TRY(cog_ln_mod_fwd(a, st));
        }
        FTMI_TRY(gemm_nt(linear_args(hn, D, rows * S, P(w.proj_w, 0), D, Kc, D, P(w.proj_b, 0), pred, Kc, V), st));
        FTMI_TRY(hy_sample_step(g, pred, x, sigmas, i, c.true_cfg, cols, st));
    }
    return 0;
}

}  // namespace ftmi
