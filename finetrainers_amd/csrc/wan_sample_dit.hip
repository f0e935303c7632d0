// Wan latent sampling: the whole denoising loop of a validation run as ONE C call (ftmi_wan_sample), for the three Wan recipes -- text-to-video, image-to-video
// (TI > 0 image tokens in attn2, 36 input channels) and control (widened patch embedding with its folded full-rank adapter).  Restates what the reference gets
// from a diffusers pipeline over the transformer it trains (finetrainers/models/wan/base_specification.py:495-529, control_specification.py:310-377), in latent
// space: text / image encoding and the VAE stay outside.
//
// Per step, on one stream, no host synchronisation:
//   wan_sample_mod                       mod [L, P B, 6, D] = float(scale_shift_table_l) + float(tproj_step)
//   patch embedding                      x0 = cols W^T + b  (NT GEMM over cols; folded adapter: wan_patch_lora_forward, the fold itself at step 0 only)
//   L x wan_lora_ffn_block_forward       the block walk of wan_dit.hip at batch P B (rows [0, B) unconditional); every block writes the SAME `saved` slot -- nothing
//                                        is kept for a backward -- and shares one scratch area; activations alternate between two [P B S, D] buffers
//   wan_ln_fwd + proj_out                the head with the step's fp32 shift / scale (one row for every sample: they share the timestep)
//   wan_sample_step                      guidance combine + Euler update on the state, bf16 copies into the columns [0, Kc) of cols
// The sampler state x fp32 [B, S, Kc] and the model input cols stay in the patch embedding's operand layout (sample_layout.hip): no patchify between steps.
// What does not depend on the state (time projection, head shift / scale, text and image rows, rotary tables, sigmas) is the caller's, computed once per call.
//
// ftmi_wan_sample_ms is the same loop (sample_loop, one body for both) whose last launch is wan_sample_step_unipc: the checkpoint's UniPC multistep scheduler, which
// is what the reference's validation pipeline runs (the trainers pass no scheduler to load_pipeline, so from_pretrained loads the checkpoint's).  Its history
// -- the last corrected state and two data predictions, three [B, S, Kc] fp32 buffers behind the Euler workspace -- never leaves the device; the two
// data-prediction pointers swap per step on the host side of the call, the step's eight coefficients come from a device table folded once on the host.
//
// Workspace: mod for the 40 blocks a launch can address (so the plan does not depend on L), the two activation buffers, pred [P B S, po], one block's saved bytes
// and one block's scratch.
#include "common.hip.h"
#include "kernels.h"
#include "lora_proj.hip.h"

namespace ftmi {

namespace {

constexpr int kMaxBlocks = 40;  // wan_sample_mod's table of scale_shift_table pointers (Wan2.1: 30 blocks at 1.3B, 40 at 14B)

struct Plan {
    size_t mod, xa, xb, pred, saved, scratch, total;
    size_t saved_bytes, scratch_bytes;
    long S, M;  // tokens per sample, model rows P B S
    ftmi_wan_lora_ffn_block_config bc;
};

int make_plan(const ftmi_wan_sample_config& c, Plan& p) {
    const ftmi_wan_sample_geometry& g = c.geo;
    if (g.B <= 0 || g.F <= 0 || g.H <= 0 || g.W <= 0 || g.pt <= 0 || g.ph <= 0 || g.pw <= 0 || c.T <= 0 || c.D <= 0 || c.steps <= 0)
        return set_error(FTMI_ERR_INVALID, "wan_sample: extents and steps must be positive");
    if (g.F % g.pt || g.H % g.ph || g.W % g.pw) return set_error(FTMI_ERR_UNSUPPORTED, "wan_sample: the latent size must be whole patches");
    if (c.L <= 0 || c.L > kMaxBlocks) return set_error(FTMI_ERR_UNSUPPORTED, "wan_sample: 1 .. 40 blocks");
    if ((c.guidance != 1.0f) != (g.P == 2) || (g.P != 1 && g.P != 2)) return set_error(FTMI_ERR_INVALID, "wan_sample: P is 2 with guidance != 1 and 1 with guidance == 1");
    if ((c.patch_fold != 0) != (g.copies == 2) || (g.copies != 1 && g.copies != 2))
        return set_error(FTMI_ERR_INVALID, "wan_sample: cols is [cols | cols] with the folded patch adapter, and only with it");
    if (g.po <= 0 || g.po % 64 || g.Kp % 64) return set_error(FTMI_ERR_UNSUPPORTED, "wan_sample: Kp and po must be multiples of 64 (GEMM)");
    p.S = (long)(g.F / g.pt) * (g.H / g.ph) * (g.W / g.pw);
    p.M = (long)g.P * g.B * p.S;
    if (p.M > 0x7fffffffL) return set_error(FTMI_ERR_UNSUPPORTED, "wan_sample: too many tokens");
    ftmi_wan_lora_ffn_block_config& b = p.bc;
    b.B = g.P * g.B; b.S = (int)p.S; b.T = c.T; b.D = c.D; b.H = c.heads; b.F = c.ffn_dim; b.eps = c.eps; b.gemm_variant = c.gemm_variant;
    b.r = c.r; b.lora_scale = c.lora_scale; b.TI = c.TI; b.TI2 = c.TI2; b.ffn = c.ffn;
    p.saved_bytes = wan_lora_ffn_block_saved_bytes(b);
    p.scratch_bytes = wan_lora_ffn_block_scratch_bytes(b);
    if (!p.saved_bytes || !p.scratch_bytes) return FTMI_ERR_UNSUPPORTED;  // (the block's planner set the message)
    Bump w;
    p.mod = w.take((size_t)kMaxBlocks * b.B * 6 * c.D * sizeof(float));
    p.xa = w.take((size_t)p.M * c.D * 2);
    p.xb = w.take((size_t)p.M * c.D * 2);
    p.pred = w.take((size_t)p.M * g.po * 2);
    p.saved = w.take(p.saved_bytes);
    p.scratch = w.take(p.scratch_bytes);
    p.total = w.off;
    return 0;
}

}  // namespace

size_t wan_sample_workspace_bytes(const ftmi_wan_sample_config& c) {
    Plan p;
    return make_plan(c, p) ? 0 : p.total;
}

namespace {

// The history of the multistep solver behind the Euler plan: last, m1, m2 fp32 [B, S, Kc] (Kc * 4 bytes is a multiple of 32: every buffer stays 16-byte aligned
// behind the 256-byte multiple p.total).
int make_ms_plan(const ftmi_wan_sample_ms_config& c, Plan& p, size_t& hist, size_t& hist_bytes, size_t& total) {
    if (c.solver != 1) return set_error(FTMI_ERR_UNSUPPORTED, "wan_sample_ms: solver 1 (UniPC) is the one multistep solver");
    FTMI_TRY(make_plan(c.base, p));
    const ftmi_wan_sample_geometry& g = c.base.geo;
    if (g.C <= 0 || (long)g.C * g.pt * g.ph * g.pw != g.po) return set_error(FTMI_ERR_INVALID, "wan_sample_ms: C pt ph pw must equal po, the width of proj_out");
    hist = p.total;
    hist_bytes = (size_t)g.B * p.S * g.po * sizeof(float);
    total = p.total + 3 * hist_bytes;
    return 0;
}

// The loop of both entry points.  step(i, pred): the launch that takes the step's prediction into the state and cols.  `need`: the entry point's workspace.
template <class Step>
int sample_loop(const ftmi_wan_sample_config& c, const Plan& p, size_t need, const ftmi_wan_sample_weights& w, bf16_t* cols, const bf16_t* tproj,
                const float* head_shift, const float* head_scale, const bf16_t* enc, const bf16_t* enc_img, const float* rope_cos, const float* rope_sin, void* ws,
                size_t ws_bytes, hipStream_t st, Step step) {
    if (ws_bytes < need) return set_error(FTMI_ERR_INVALID, "wan_sample: workspace too small (ftmi_wan_sample_workspace_bytes)");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return set_error(FTMI_ERR_INVALID, "wan_sample: the workspace must be 256-byte aligned");
    if (!w.blocks || !w.patch_w || !w.proj_w) return set_error(FTMI_ERR_INVALID, "wan_sample: weights missing");
    if (c.TI > 0 && (!w.img_params || !enc_img)) return set_error(FTMI_ERR_INVALID, "wan_sample: image tokens without their parameters");
    if (c.patch_fold && (!w.patch_lora_a || !w.patch_lora_b || !w.patch_dw || !w.patch_w2)) return set_error(FTMI_ERR_INVALID, "wan_sample: folded patch adapter without its buffers");
    const ftmi_wan_sample_geometry& g = c.geo;
    const int D = c.D, L = c.L, rows = g.P * g.B, M = (int)p.M;
    ftmi_wan_block_config base;
    base.B = rows; base.S = (int)p.S; base.T = c.T; base.D = D; base.H = c.heads; base.F = c.ffn_dim; base.eps = c.eps; base.gemm_variant = c.gemm_variant;
    const size_t table_off = wan_block_param_elements(base) - 6 * (size_t)D;  // scale_shift_table is the last entry of a block's flat buffer
    const bf16_t* tables[kMaxBlocks];
    for (int l = 0; l < L; ++l) {
        if (!w.blocks[l].base.params) return set_error(FTMI_ERR_INVALID, "wan_sample: a block without parameters");
        if (c.TI > 0 && !w.img_params[l]) return set_error(FTMI_ERR_INVALID, "wan_sample: a block without its image-context parameters");
        tables[l] = reinterpret_cast<const bf16_t*>(w.blocks[l].base.params) + table_off;
    }
    float* mod = WF(ws, p.mod);
    bf16_t *xa = W(ws, p.xa), *xb = W(ws, p.xb), *pred = W(ws, p.pred);
    void *saved = W(ws, p.saved), *scratch = W(ws, p.scratch);
    const long ld = (long)g.copies * g.Kp;
    for (int i = 0; i < c.steps; ++i) {
        FTMI_TRY(wan_sample_mod(tables, L, tproj + (size_t)i * 6 * D, mod, rows, D, st));
        if (c.patch_fold) {
            ftmi_wan_patch_lora_config pc;
            pc.M = M; pc.D = D; pc.Kp = g.Kp; pc.r = c.patch_r; pc.s = c.patch_scale; pc.gemm_variant = c.gemm_variant; pc.refold = i == 0;
            FTMI_TRY(wan_patch_lora_forward(pc, (const bf16_t*)w.patch_w, (const bf16_t*)w.patch_b, w.patch_lora_a, w.patch_lora_b, cols, w.patch_dw, (bf16_t*)w.patch_w2, xa, st));
        } else {
            FTMI_TRY(gemm_nt(linear_args(cols, ld, M, (const bf16_t*)w.patch_w, g.Kp, D, g.Kp, (const bf16_t*)w.patch_b, xa, D, c.gemm_variant), st));
        }
        bf16_t *cur = xa, *nxt = xb;
        for (int l = 0; l < L; ++l) {
            FTMI_TRY(wan_lora_ffn_block_forward(p.bc, w.blocks[l], c.TI > 0 ? (const bf16_t*)w.img_params[l] : nullptr, cur, enc, c.TI > 0 ? enc_img : nullptr,
                                                mod + (size_t)l * rows * 6 * D, rope_cos, rope_sin, nxt, saved, p.saved_bytes, scratch, p.scratch_bytes, st));
            bf16_t* t = cur; cur = nxt; nxt = t;
        }
        {  // the head: LN with the step's shift / scale (sample stride 0: the rows share the timestep), then proj_out
            WanRowArgs a;
            a.x = cur; a.ld_x = D; a.y = nxt; a.ld_y = D; a.rows = M; a.D = D; a.rows_per_batch = (int)p.S; a.eps = c.eps;
            a.shift = head_shift + (size_t)i * D; a.scale = head_scale + (size_t)i * D; a.mod_bstride = 0;
            FTMI_TRY(wan_ln_fwd(a, st));
            FTMI_TRY(gemm_nt(linear_args(nxt, D, M, (const bf16_t*)w.proj_w, D, g.po, D, (const bf16_t*)w.proj_b, pred, g.po, c.gemm_variant), st));
        }
        FTMI_TRY(step(i, pred));
    }
    return 0;
}

}  // namespace

int wan_sample(const ftmi_wan_sample_config& c, const ftmi_wan_sample_weights& w, bf16_t* cols, float* x, const bf16_t* tproj, const float* head_shift,
               const float* head_scale, const bf16_t* enc, const bf16_t* enc_img, const float* rope_cos, const float* rope_sin, const float* sigmas, void* ws,
               size_t ws_bytes, hipStream_t st) {
    Plan p;
    FTMI_TRY(make_plan(c, p));
    return sample_loop(c, p, p.total, w, cols, tproj, head_shift, head_scale, enc, enc_img, rope_cos, rope_sin, ws, ws_bytes, st, [&](int i, const bf16_t* pred) {
        return wan_sample_step(c.geo, pred, x, sigmas + i, sigmas + i + 1, 0, c.guidance, cols, st);
    });
}

size_t wan_sample_ms_workspace_bytes(const ftmi_wan_sample_ms_config& c) {
    Plan p;
    size_t hist, hist_bytes, total;
    return make_ms_plan(c, p, hist, hist_bytes, total) ? 0 : total;
}

int wan_sample_ms(const ftmi_wan_sample_ms_config& c, const ftmi_wan_sample_weights& w, bf16_t* cols, float* x, const bf16_t* tproj, const float* head_shift,
                  const float* head_scale, const bf16_t* enc, const bf16_t* enc_img, const float* rope_cos, const float* rope_sin, const float* coef,
                  const float* sigmas, void* ws, size_t ws_bytes, hipStream_t st) {
    Plan p;
    size_t hist, hist_bytes, total;
    FTMI_TRY(make_ms_plan(c, p, hist, hist_bytes, total));
    char* h = reinterpret_cast<char*>(ws) + hist;
    float* last = reinterpret_cast<float*>(h);
    float *m1 = reinterpret_cast<float*>(h + hist_bytes), *m2 = reinterpret_cast<float*>(h + 2 * hist_bytes);  // step i reads m_{i-1}, m_{i-2} and writes m_i over m2
    return sample_loop(c.base, p, total, w, cols, tproj, head_shift, head_scale, enc, enc_img, rope_cos, rope_sin, ws, ws_bytes, st, [&](int i, const bf16_t* pred) {
        const int rc = wan_sample_step_unipc(c.base.geo, pred, x, last, m1, m2, coef + (size_t)i * 8, sigmas + i, c.base.guidance, cols, st);
        float* t = m1; m1 = m2; m2 = t;
        return rc;
    });
}

}  // namespace ftmi
