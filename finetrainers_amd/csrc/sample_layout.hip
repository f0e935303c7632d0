// Wan, CogVideoX and HunyuanVideo latent sampling, the kernels around the DiT forward of a denoising loop (the orchestrators are wan_sample in
// wan_sample_dit.hip, cog_sample in cog_dit.hip, next to the block walk, and hy_sample in hy_sample_dit.hip).
//
// The sampler state lives in the patch embedding's OPERAND layout, so a step needs no patchify / un-patchify:
//   state  x     fp32 [B, S, Kc]       Kc = C pt ph pw columns in the patch embedding's order (c, pt, ph, pw): column c pv + dt ph pw + dy pw + dx, pv = pt ph pw;
//                                      S = (F / pt)(H / ph)(W / pw) tokens in (f, h, w) order
//   input  cols  bf16 [P B S, ld]      the patch-embedding GEMM's operand.  ld = copies Kp, Kp the stored patch width; columns [0, Kc) of every copy are bf16(x),
//                                      the others (extra channels, then +0 padding) are constant over the loop.  P = 2 row groups with guidance (rows [0, B S)
//                                      unconditional, [B S, 2 B S) conditional), 1 without.
//   output pred  bf16 [P B, S, Kc]     what proj_out writes.
// One layout (struct Lay), two models:
//                                      Wan                                                     CogVideoX
//   latent tensor                      [B, C, F, H, W]                                         [B, F, C, H, W] (frames BEFORE channels): Lay::sc, sf swapped
//   patch                              (pt, ph, pw)                                            (pt, p, p), pt <= 2
//   extra bf16 channels, copies, Kp    Cx (I2V: mask + condition; control), 1 or 2 ([cols |    none: Cx = 0, copies = 1, Kp = ld = Kc
//                                      cols], the folded patch adapter), 64 / 192 / 128
//   leading frames dropped by finish   none: drop = 0                                          drop < pt (what the pipeline pads at the front for patch_size_t)
//   affine of finish                   per channel, x * std[c] + mean[c]                       scalar, x * k
//   column order of pred               (pt, ph, pw, c): permuted through the LDS in the step   the state's: the step is a row-major stream
//   update of the step                 flow-match Euler, x <- fma(dt, v, x)                    DDIM (v-prediction, eta = 0), x <- fma(cx, x, cv * v)
//
// sample_init_kernel: latents fp32 (+ extra bf16 [B, Cx, F, H, W]) -> x (exact) and every row group and copy of cols.  One workgroup per row of patches
//   (b, f', h'): the contiguous piece of a channel inside it is the run of ph W elements of one (channel, frame) plane; the C pt runs (and the Cx pt of the extra
//   channels) are staged in the LDS through the aligned 16-byte vectors that cover them, then every thread gathers 8 columns of one token and stores them as
//   vectors.  Bytes moved per state element: 4 read, 4 + 2 P copies written; per extra element 2 read, 2 P copies written.
// wan_sample_step / cog_sample_step: classifier-free-guidance combine (sample_step.hip.h) + the model's update of one step, one pass, all fp32; bf16(x) (round
//   to nearest even) goes to columns [0, Kc) of every row group and copy of cols.  pred == nullptr: no update, only the copies.
//   Wan: dt = sigma_next - sigma, read from the device; the arithmetic is cfg_euler_step's (ltx_sample.hip), which restates [upstream, unpinned]
//   FlowMatchEulerDiscreteScheduler.step after the pipeline's noise_uncond + guidance_scale * (noise_pred - noise_uncond).  A thread combines 16 bytes of each
//   half of pred in pred's order and hands v to the thread that owns the state columns through the LDS: state column c pv + p is pred column p C + c, so a
//   token's columns are permuted on chip and every global access stays a 16-byte vector.  Bytes moved per element of x: 12 + 2 P copies with guidance (read
//   u 2 + c 2 + x 4, write x 4 + cols): 16 for T2V / I2V, 20 with the folded patch adapter; 10 + 2 copies without guidance: 12 / 14.
//   Wan, multistep (wan_sample_step_unipc): the checkpoint's UniPCMultistepScheduler (data prediction, flow sigmas, bh2, order <= 2), folded on the host into eight
//   numbers per step (finetrainers_amd/wan/sampler.py wan_unipc_tables; the step is linear in the state, the last corrected state and three data predictions).
//   Same mapping, combine and on-chip permutation as the Euler step; per element, all fp32, one rounding per operation:
//       m  = fma(-sigma, v, x)                                          the data prediction of this step
//       x~ = c_x x + c_l last + c_1 m1 + c_2 m2 + c_t m                  the corrector (c_x = 1, the others 0: none)
//       x' = p_x x~ + p_0 m + p_1 m1                                     the predictor
//   each sum a product followed by fmas in the order written; a term whose coefficient is 0 is neither loaded nor added (step 0 has no history, and 0 * NaN of
//   an uninitialised workspace must not reach x): the coefficients are one row of a device table, so the branches are uniform over the launch.  x' goes to x and,
//   as bf16, to cols; x~ to last; m over m2, the OLDER of the two history buffers (the caller swaps m1 / m2 after the step).  Bytes moved per element of x with
//   guidance, full order-2 row: read u 2 + c 2 + x 4 + last 4 + m1 4 + m2 4 = 20, write x 4 + last 4 + m 4 + 2 P copies = 16 at P = 2, copies = 1: 36 (40 with
//   the folded patch adapter) against Euler's 16; step 0 reads 8 and the last step writes the same 16.
//   CogVideoX: (cx, cv) are the step's two numbers of the host-folded scheduler ([upstream, unpinned] CogVideoXDDIMScheduler.step is linear in (x, v):
//   finetrainers_amd/cogvideox/sampler.py cog_ddim_tables), read from a device table.  A thread owns 8 consecutive elements; the last workgroup's tail is
//   masked.  Bytes moved per element of x: 12 + 2 P with guidance = 16; 10 + 2 = 12 without.
//   CogVideoX, multistep (cog_sample_step_dpm): the 5b / 1.5 checkpoints' [upstream, unpinned] CogVideoXDPMScheduler, a second-order multistep SDE solver that
//   keeps the previous step's x0 prediction and adds fresh noise z at every step but the last, folded on the host into eight numbers per step
//   (finetrainers_amd/cogvideox/sampler.py cog_dpm_tables): row = (sa, sb, m0, e0, e1, mn, g, 0), g the step's guidance scale.  The same stream; per element:
//       x0 = fma(-sb, v, sa x)                                          the data prediction of this step
//       x' = m0 x;  x' = fma(e0, x0, x');  fma(e1, old, x');  fma(mn, z, x')
//   a term whose coefficient is 0 is neither loaded nor added (old is uninitialised at step 0, the last step has no noise).  x' goes to x and, as bf16, to cols;
//   x0 to old.  Bytes moved per element of x with guidance, full row: read u 2 + c 2 + x 4 + old 4 + z 4 = 16, write x 4 + old 4 + 2 P copies = 12: 28.
//   cog_sample_pack: init's permutation over n noise tensors at once (the per-step noise of that solver, into the state's layout): sample_init_kernel over n B
//   samples with no row group of cols to write.
//   HunyuanVideo (hy_sample_step): CogVideoX's layout over [B, C, F, H, W] latents (Lay::sc, sf as Wan's; Cx = 0, copies = 1, Kp = Kc, drop = 0; finish is
//   the scalar affine with k = 1 / scaling_factor) and Wan's update: dt = sigmas[step + 1] - sigmas[step] read from the device table, x <- fma(dt, v, x).  A
//   row-major stream like CogVideoX's.  Bytes moved per element of x: 10 without true CFG (pred 2 + x 4 read, x 4 + cols 2 written), 16 with.
// sample_finish_kernel: x fp32 [B, S, Kc] -> latents bf16 = bf16(affine(x)), the inverse permutation of init; the first `drop` frames are not written.  Wan's std
//   is the VAE's REAL standard deviation -- not the 1 / std the training processors hand over (finetrainers/models/wan/base_specification.py multiplies by
//   latents_std = 1 / std when it normalises).  The two affines are two instantiations, not two data sets: v * k + 0 would turn -0 into +0.  16-byte reads along
//   the token columns, 16-byte writes along the runs when they are 16-byte aligned (ph W % 8 == 0), element stores otherwise.  Bytes moved per element: 4 read
//   + 2 written.
// wan_sample_mod: the fp32 modulation of all L blocks for ONE step, mod [L, rows, 6, D] = float(scale_shift_table_l) + float(tproj_step) (the expression of
//   finetrainers_amd/wan/block.py _fwd), every row of a step sharing one timestep: there is no [steps, L, ...] table.  Bytes per output element: 4 written, 4 / rows read.
#include "common.hip.h"
#include "kernels.h"
#include "sample_step.hip.h"

namespace ftmi {

namespace {

// what the layout kernels share, derived once on the host (wan_lay / cog_lay, lay_derive)
struct Lay {
    int B, C, Cx, F, H, W, pt, ph, pw;
    long sc, sf;  // element strides of a channel / a frame of the latent tensor: (F H W, H W) for [B, C, F, H, W], (H W, C H W) for [B, F, C, H, W].  The extra
                  // channels (their own channel count) exist in the first order only, dropped frames (another frame count) in the second: sc, sf hold for them too
    int Kp, copies, P, drop;
    int pv, Kc, Kx, ld;
    int fpn, hpn, wpn;  // patches along F, H, W
    long S;             // tokens per sample
    int seg_len;        // ph W: one contiguous run of a (channel, frame) plane inside a row of patches
    int pitch_f, pitch_h;  // LDS elements per run: fp32 (multiple of 4) / bf16 (multiple of 8)
};

// state column k -> (run = c pt + dt, offset inside the run for token w of the row of patches)
// (nothing here is negative, and an unsigned division is about two thirds of the instructions of a signed one)
FTMI_DEVICE void col_src(const Lay& g, int k, int w, int& run, int& off) {
    const unsigned pp = g.ph * g.pw, r = (unsigned)k / pp, rem = k - r * pp;
    const unsigned dy = rem / g.pw, dx = rem - dy * g.pw;
    run = r;
    off = dy * g.W + w * g.pw + dx;
}

// first element of run (c, dt) of the row of patches (b, f', h') in a tensor of nch channels and `frames` frames whose frame 0 is frame `first` of the grid
FTMI_DEVICE long run_start(const Lay& g, int nch, int b, int fp, int hp, int run, int frames, int first) {
    const int c = (unsigned)run / (unsigned)g.pt, dt = run - c * g.pt;
    return (long)b * nch * frames * g.H * g.W + c * g.sc + (fp * g.pt + dt - first) * g.sf + (long)hp * g.ph * g.W;
}

FTMI_DEVICE void block_coords(const Lay& g, int& b, int& fp, int& hp) {
    int t = blockIdx.x;
    hp = t % g.hpn; t /= g.hpn;
    fp = t % g.fpn;
    b = t / g.fpn;
}

// grid B f' h' workgroups of 256; dynamic LDS: C pt pitch_f floats, then Cx pt pitch_h bf16
__global__ __launch_bounds__(256) void sample_init_kernel(Lay g, const float* __restrict__ lat, const bf16_t* __restrict__ extra, float* __restrict__ x,
                                                          bf16_t* __restrict__ cols) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lf = reinterpret_cast<float*>(smem);
    bf16_t* lh = reinterpret_cast<bf16_t*>(smem + (size_t)g.C * g.pt * g.pitch_f * 4);
    int b, fp, hp;
    block_coords(g, b, fp, hp);
    const int tid = threadIdx.x;
    {  // the runs of the latents, through the aligned 16-byte vectors that cover them (the tensor is a whole number of vectors: the cover stays inside it)
        const int nrun = g.C * g.pt, vpr = g.pitch_f / 4;
        for (int idx = tid; idx < nrun * vpr; idx += 256) {
            const int run = idx / vpr, vi = idx - run * vpr;
            const long start = run_start(g, g.C, b, fp, hp, run, g.F, 0);
            const long gv = (start >> 2) + vi;
            if (gv < ((start + g.seg_len + 3) >> 2)) reinterpret_cast<f32x4*>(lf)[idx] = reinterpret_cast<const f32x4*>(lat)[gv];
        }
    }
    if (g.Cx > 0) {
        const int nrun = g.Cx * g.pt, vpr = g.pitch_h / 8;
        for (int idx = tid; idx < nrun * vpr; idx += 256) {
            const int run = idx / vpr, vi = idx - run * vpr;
            const long start = run_start(g, g.Cx, b, fp, hp, run, g.F, 0);
            const long gv = (start >> 3) + vi;
            if (gv < ((start + g.seg_len + 7) >> 3)) reinterpret_cast<u32x4*>(lh)[idx] = reinterpret_cast<const u32x4*>(extra)[gv];
        }
    }
    __syncthreads();
    // out: wpn tokens x Kp / 8 vectors of 8 columns; element e of a run sits (start mod vector) + e into its LDS slot
    const int vpt = g.Kp / 8;
    for (int idx = tid; idx < g.wpn * vpt; idx += 256) {
        const int w = idx / vpt, k0 = (idx - w * vpt) * 8;
        const long t = ((long)fp * g.hpn + hp) * g.wpn + w;
        u32x4 o = {0u, 0u, 0u, 0u};
        if (k0 < g.Kc) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                int run, off;
                col_src(g, k0 + e, w, run, off);
                v[e] = lf[run * g.pitch_f + (int)(run_start(g, g.C, b, fp, hp, run, g.F, 0) & 3) + off];
            }
            f32x4* xp = reinterpret_cast<f32x4*>(x + ((long)b * g.S + t) * g.Kc + k0);
            xp[0] = f32x4{v[0], v[1], v[2], v[3]};
            xp[1] = f32x4{v[4], v[5], v[6], v[7]};
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = pack2bf(v[2 * e], v[2 * e + 1]);
        } else if (k0 < g.Kc + g.Kx) {
            bf16_t h[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                int run, off;
                col_src(g, k0 - g.Kc + e, w, run, off);
                h[e] = lh[run * g.pitch_h + (int)(run_start(g, g.Cx, b, fp, hp, run, g.F, 0) & 7) + off];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (uint32_t)h[2 * e] | ((uint32_t)h[2 * e + 1] << 16);
        }
        for (int p = 0; p < g.P; ++p)
            for (int cp = 0; cp < g.copies; ++cp)
                *reinterpret_cast<u32x4*>(cols + (((long)p * g.B + b) * g.S + t) * g.ld + (long)cp * g.Kp + k0) = o;
    }
}

// n8 = B S Kc / 8 vectors; a workgroup's 2048 elements are whole tokens (2048 % Kc == 0).  kCfg: two row groups (pred has an unconditional half).
template <bool kCfg>
__global__ __launch_bounds__(256) void wan_sample_step_kernel(Lay g, const bf16_t* __restrict__ pred, float* __restrict__ x, const float* __restrict__ sigma,
                                                              const float* __restrict__ sigma_next, long sig_stride, float gd, bf16_t* __restrict__ cols, long n8) {
    __shared__ __attribute__((aligned(16))) float sv[2048];  // the combined prediction of the workgroup's tokens, in the STATE's column order
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * 256 + tid;
    const bool live = i < n8;
    const int vpt = g.Kc / 8;
    const long tok = i / vpt;
    const int j0 = (int)(i - tok * vpt) * 8;
    if (pred) {
        if (live) {
            float v[8];
            cfg_combine8<kCfg>(pred, i, n8, gd, v);
            const int base = (tid / vpt) * g.Kc;
#pragma unroll
            for (int e = 0; e < 8; ++e) {  // pred column j = p C + c  ->  state column c pv + p
                const int j = j0 + e;
                sv[base + (j % g.C) * g.pv + j / g.C] = v[e];
            }
        }
        __syncthreads();
    }
    if (!live) return;
    f32x4* xp = reinterpret_cast<f32x4*>(x) + 2 * i;
    f32x4 x0 = xp[0], x1 = xp[1];
    float xv[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    const long b = tok / g.S, t = tok - b * g.S;
    if (pred) {
        const float dt = sigma_next[b * sig_stride] - sigma[b * sig_stride];
        const f32x4 v0 = reinterpret_cast<const f32x4*>(sv)[2 * tid], v1 = reinterpret_cast<const f32x4*>(sv)[2 * tid + 1];
        const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = __builtin_fmaf(dt, v[e], xv[e]);
        xp[0] = f32x4{xv[0], xv[1], xv[2], xv[3]};
        xp[1] = f32x4{xv[4], xv[5], xv[6], xv[7]};
    }
    if (cols)
        for (int cp = 0; cp < g.copies; ++cp) store_groups8<kCfg>(cols, xv, (b * g.S + t) * g.ld + (long)cp * g.Kp + j0, (long)g.B * g.S * g.ld);
}

// acc (+)= c val over a thread's 8 elements, one rounding per element (the first term is a product, every further one an fma).  A zero coefficient leaves its
// term out: the caller does not load that buffer either, whose values may be uninitialised (0 * NaN).  c is one value per launch: the branch is uniform.
FTMI_DEVICE void lin_term8(float c, const float* val, float* acc, bool& first) {
    if (c == 0.0f) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = first ? c * val[e] : __builtin_fmaf(c, val[e], acc[e]);
    first = false;
}

FTMI_DEVICE void load8(const float* __restrict__ p, long i, float* v) {
    const f32x4 a = reinterpret_cast<const f32x4*>(p)[2 * i], b = reinterpret_cast<const f32x4*>(p)[2 * i + 1];
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}

FTMI_DEVICE void store8(float* __restrict__ p, long i, const float* v) {
    reinterpret_cast<f32x4*>(p)[2 * i] = f32x4{v[0], v[1], v[2], v[3]};
    reinterpret_cast<f32x4*>(p)[2 * i + 1] = f32x4{v[4], v[5], v[6], v[7]};
}

// The multistep step: wan_sample_step_kernel's thread-to-data mapping (n8 = B S Kc / 8 vectors, a workgroup's 2048 elements are whole tokens, v through the
// LDS into the state's column order) with the UniPC update of the file header.  coef: the step's row (c_x, c_l, c_1, c_2, c_t, p_x, p_0, p_1), sigma: its sigma.
// last / m1 / m2 fp32 [B, S, Kc] like x; m2 (the OLDER history buffer) receives m: vector i of it is read and written by thread i alone.
template <bool kCfg>
__global__ __launch_bounds__(256) void wan_sample_step_unipc_kernel(Lay g, const bf16_t* __restrict__ pred, float* __restrict__ x, float* __restrict__ last,
                                                                    const float* __restrict__ m1, float* __restrict__ m2, const float* __restrict__ coef,
                                                                    const float* __restrict__ sigma, float gd, bf16_t* __restrict__ cols, long n8) {
    __shared__ __attribute__((aligned(16))) float sv[2048];  // the combined prediction of the workgroup's tokens, in the STATE's column order
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * 256 + tid;
    const bool live = i < n8;
    const int vpt = g.Kc / 8;
    const long tok = i / vpt;
    const int j0 = (int)(i - tok * vpt) * 8;
    if (live) {
        float v[8];
        cfg_combine8<kCfg>(pred, i, n8, gd, v);
        const int base = (tid / vpt) * g.Kc;
#pragma unroll
        for (int e = 0; e < 8; ++e) {  // pred column j = p C + c  ->  state column c pv + p
            const int j = j0 + e;
            sv[base + (j % g.C) * g.pv + j / g.C] = v[e];
        }
    }
    __syncthreads();
    if (!live) return;
    const float cx = coef[0], cl = coef[1], c1 = coef[2], c2 = coef[3], ct = coef[4], px = coef[5], p0 = coef[6], p1 = coef[7], sg = sigma[0];
    float xv[8], v[8], m[8], lv[8], h1[8], h2[8];
    load8(x, i, xv);
    load8(sv, tid, v);
    if (cl != 0.0f) load8(last, i, lv);
    if (c1 != 0.0f || p1 != 0.0f) load8(m1, i, h1);
    if (c2 != 0.0f) load8(m2, i, h2);
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = __builtin_fmaf(-sg, v[e], xv[e]);
    float xt[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, xn[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool first = true;
    lin_term8(cx, xv, xt, first);
    lin_term8(cl, lv, xt, first);
    lin_term8(c1, h1, xt, first);
    lin_term8(c2, h2, xt, first);
    lin_term8(ct, m, xt, first);
    first = true;
    lin_term8(px, xt, xn, first);
    lin_term8(p0, m, xn, first);
    lin_term8(p1, h1, xn, first);
    store8(x, i, xn);
    store8(last, i, xt);
    store8(m2, i, m);
    if (cols) {
        const long b = tok / g.S, t = tok - b * g.S;
        for (int cp = 0; cp < g.copies; ++cp) store_groups8<kCfg>(cols, xn, (b * g.S + t) * g.ld + (long)cp * g.Kp + j0, (long)g.B * g.S * g.ld);
    }
}

// n8 = B S Kc / 8 vectors, one per thread; grid ceil(n8 / 256).  kCfg: two row groups (pred has an unconditional half).
template <bool kCfg>
__global__ __launch_bounds__(256) void cog_sample_step_kernel(const bf16_t* __restrict__ pred, float* __restrict__ x, const float* __restrict__ coef, int step,
                                                              float gd, bf16_t* __restrict__ cols, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    f32x4* xp = reinterpret_cast<f32x4*>(x) + 2 * i;
    const f32x4 x0 = xp[0], x1 = xp[1];
    float xv[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    if (pred) {
        const float cx = coef[2 * step], cv = coef[2 * step + 1];
        float v[8];
        cfg_combine8<kCfg>(pred, i, n8, gd, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = __builtin_fmaf(cx, xv[e], cv * v[e]);
        xp[0] = f32x4{xv[0], xv[1], xv[2], xv[3]};
        xp[1] = f32x4{xv[4], xv[5], xv[6], xv[7]};
    }
    if (cols) store_groups8<kCfg>(cols, xv, 8 * i, 8 * n8);
}

// The multistep step of CogVideoX: cog_sample_step_kernel's stream (n8 = B S Kc / 8 vectors, one per thread) with the DPM update of the file header.  row: the
// step's eight numbers (sa, sb, m0, e0, e1, mn, g, 0) on the device.  old / z fp32 [B, S, Kc] like x; vector i of x and old is read and written by thread i alone.
// A zero e1 / mn leaves its term out and its buffer unread (lin_term8); z == nullptr is read as mn == 0.
template <bool kCfg>
__global__ __launch_bounds__(256) void cog_sample_step_dpm_kernel(const bf16_t* __restrict__ pred, float* __restrict__ x, float* __restrict__ old,
                                                                  const float* __restrict__ z, const float* __restrict__ row, bf16_t* __restrict__ cols, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const float sa = row[0], sb = row[1], m0 = row[2], e0 = row[3], e1 = row[4], mn = z ? row[5] : 0.0f, gd = row[6];
    float xv[8], v[8], p0[8], ov[8], zv[8], a[8];
    load8(x, i, xv);
    cfg_combine8<kCfg>(pred, i, n8, gd, v);
    if (e1 != 0.0f) load8(old, i, ov);
    if (mn != 0.0f) load8(z, i, zv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        p0[e] = __builtin_fmaf(-sb, v[e], sa * xv[e]);
        a[e] = __builtin_fmaf(e0, p0[e], m0 * xv[e]);
    }
    bool first = false;
    lin_term8(e1, ov, a, first);
    lin_term8(mn, zv, a, first);
    store8(x, i, a);
    store8(old, i, p0);
    if (cols) store_groups8<kCfg>(cols, a, 8 * i, 8 * n8);
}

// n8 = B S Kc / 8 vectors, one per thread; grid ceil(n8 / 256).  kCfg: two row groups (pred has an unconditional half).
template <bool kCfg>
__global__ __launch_bounds__(256) void hy_sample_step_kernel(const bf16_t* __restrict__ pred, float* __restrict__ x, const float* __restrict__ sigmas, int step,
                                                             float gd, bf16_t* __restrict__ cols, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    f32x4* xp = reinterpret_cast<f32x4*>(x) + 2 * i;
    const f32x4 x0 = xp[0], x1 = xp[1];
    float xv[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    if (pred) {
        const float dt = sigmas[step + 1] - sigmas[step];
        float v[8];
        cfg_combine8<kCfg>(pred, i, n8, gd, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = __builtin_fmaf(dt, v[e], xv[e]);
        xp[0] = f32x4{xv[0], xv[1], xv[2], xv[3]};
        xp[1] = f32x4{xv[4], xv[5], xv[6], xv[7]};
    }
    if (cols) store_groups8<kCfg>(cols, xv, 8 * i, 8 * n8);
}

struct ChannelAffine {  // Wan
    const float* __restrict__ mean;
    const float* __restrict__ std_;
    FTMI_DEVICE float operator()(float v, int c) const { return v * std_[c] + mean[c]; }
};
struct ScalarAffine {  // CogVideoX
    float k;
    FTMI_DEVICE float operator()(float v, int) const { return v * k; }
};

// grid B f' h' workgroups of 256; dynamic LDS: C pt pitch_h bf16, [run][dy W + w pw + dx]
template <class Affine>
__global__ __launch_bounds__(256) void sample_finish_kernel(Lay g, const float* __restrict__ x, Affine affine, bf16_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* lh = reinterpret_cast<bf16_t*>(smem);
    int b, fp, hp;
    block_coords(g, b, fp, hp);
    const int tid = threadIdx.x;
    const long t0 = ((long)fp * g.hpn + hp) * g.wpn;
    const int vpt = g.Kc / 4;
    for (int idx = tid; idx < g.wpn * vpt; idx += 256) {  // in: wpn tokens x Kc / 4 vectors of 4 state columns, one contiguous stretch of x
        const int w = idx / vpt, k0 = (idx - w * vpt) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((long)b * g.S + t0 + w) * g.Kc + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int run, off;
            col_src(g, k0 + e, w, run, off);
            lh[run * g.pitch_h + off] = f2bf(affine(v[e], (k0 + e) / g.pv));
        }
    }
    __syncthreads();
    const int nrun = g.C * g.pt, frames = g.F - g.drop;
    auto kept = [&](int run) { return fp * g.pt + (run % g.pt) >= g.drop; };  // the run's frame is not one of the dropped leading frames
    if ((g.seg_len & 7) == 0) {  // every run starts and ends on a 16-byte boundary
        const int vpr = g.seg_len / 8;
        for (int idx = tid; idx < nrun * vpr; idx += 256) {
            const int run = idx / vpr, vi = idx - run * vpr;
            if (kept(run)) *reinterpret_cast<u32x4*>(out + run_start(g, g.C, b, fp, hp, run, frames, g.drop) + vi * 8) = *reinterpret_cast<const u32x4*>(lh + run * g.pitch_h + vi * 8);
        }
    } else {  // the runs are not 16-byte aligned: element stores
        for (int idx = tid; idx < nrun * g.seg_len; idx += 256) {
            const int run = idx / g.seg_len, e = idx - run * g.seg_len;
            if (kept(run)) out[run_start(g, g.C, b, fp, hp, run, frames, g.drop) + e] = lh[run * g.pitch_h + e];
        }
    }
}

constexpr int kModMaxBlocks = 40;  // the deepest Wan model (14B) has 40 blocks; the pointers travel as a kernel argument
struct ModArgs {
    const bf16_t* table[kModMaxBlocks];
    const bf16_t* tproj;
    float* out;
    int rows, n8;  // n8 = 6 D / 8
};

// grid (ceil(n8 / 256), L)
__global__ __launch_bounds__(256) void wan_sample_mod_kernel(ModArgs a) {
    const int v = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
    if (v >= a.n8) return;
    float tb[8], tp[8];
    unpack8(reinterpret_cast<const u32x4*>(a.table[l])[v], tb);
    unpack8(reinterpret_cast<const u32x4*>(a.tproj)[v], tp);
    const f32x4 s0 = {tb[0] + tp[0], tb[1] + tp[1], tb[2] + tp[2], tb[3] + tp[3]}, s1 = {tb[4] + tp[4], tb[5] + tp[5], tb[6] + tp[6], tb[7] + tp[7]};
    for (int r = 0; r < a.rows; ++r) {
        f32x4* op = reinterpret_cast<f32x4*>(a.out) + (((long)l * a.rows + r) * a.n8 + v) * 2;
        op[0] = s0;
        op[1] = s1;
    }
}

int fail(const char* what, int code, const char* why) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", what, why);
    return set_error(code, msg);
}

// The derived fields of a layout whose given ones (B .. drop) passed their model's checks, and the bounds of the grids.
int lay_derive(Lay& l, const char* what) {
    l.pv = l.pt * l.ph * l.pw; l.Kc = l.C * l.pv; l.Kx = l.Cx * l.pv; l.ld = l.copies * l.Kp;
    l.fpn = l.F / l.pt; l.hpn = l.H / l.ph; l.wpn = l.W / l.pw;
    l.S = (long)l.fpn * l.hpn * l.wpn;
    l.seg_len = l.ph * l.W;
    l.pitch_f = 4 * ((l.seg_len + 3) / 4 + 1);
    l.pitch_h = 8 * ((l.seg_len + 7) / 8 + 1);
    if ((long)l.B * l.fpn * l.hpn > 0x7fffffffL || (long)l.P * l.B * l.S * l.ld / 8 > 0x7fffffffL * 256L) return fail(what, FTMI_ERR_UNSUPPORTED, "too many elements for one launch");
    return 0;
}

// The dynamic LDS of init (the fp32 runs of the latents and the bf16 runs of the extra channels, both read as whole 16-byte vectors) or finish (bf16 runs).
int launch_limits(const Lay& l, bool init, const char* what, size_t& lds) {
    const long per = (long)l.F * l.H * l.W;
    if (init && (((long)l.B * l.C * per) % 4 || ((long)l.B * l.Cx * per) % 8)) return fail(what, FTMI_ERR_UNSUPPORTED, "the latents must be a whole number of 16-byte vectors");
    lds = init ? (size_t)l.C * l.pt * l.pitch_f * 4 + (size_t)l.Cx * l.pt * l.pitch_h * 2 : (size_t)l.C * l.pt * l.pitch_h * 2;
    if (lds > 64 * 1024) return fail(what, FTMI_ERR_UNSUPPORTED, "a row of patches does not fit the LDS");
    return 0;
}

int wan_lay(const ftmi_wan_sample_geometry& g, const char* what, Lay& l) {
    if (g.B <= 0 || g.C <= 0 || g.Cx < 0 || g.F <= 0 || g.H <= 0 || g.W <= 0 || g.pt <= 0 || g.ph <= 0 || g.pw <= 0 || g.Kp <= 0)
        return fail(what, FTMI_ERR_INVALID, "extents must be positive");
    if (g.copies != 1 && g.copies != 2) return fail(what, FTMI_ERR_INVALID, "copies is 1, or 2 for [cols | cols]");
    if (g.P != 1 && g.P != 2) return fail(what, FTMI_ERR_INVALID, "P is 2 with guidance, 1 without");
    if (g.F % g.pt || g.H % g.ph || g.W % g.pw) return fail(what, FTMI_ERR_UNSUPPORTED, "the latent size must be whole patches");
    const long pv = (long)g.pt * g.ph * g.pw, Kc = g.C * pv, Kx = g.Cx * pv, ld = (long)g.copies * g.Kp;
    if (Kc > 2048 || Kx > 65536 || g.Kp > 65536) return fail(what, FTMI_ERR_UNSUPPORTED, "patch too wide");
    if (Kc % 8 || Kx % 8) return fail(what, FTMI_ERR_UNSUPPORTED, "C pt ph pw (and the extra channels' columns) must be multiples of 8 (16-byte vectors)");
    if (g.Kp % 8 || ld % 8) return fail(what, FTMI_ERR_UNSUPPORTED, "the row stride ld must be a multiple of 8 (16-byte vectors)");
    if (Kc != g.po) return fail(what, FTMI_ERR_INVALID, "C pt ph pw must equal po, the width of proj_out");
    if (Kc + Kx > g.Kp) return fail(what, FTMI_ERR_INVALID, "the state and extra columns do not fit the stored patch width Kp");
    if (2048 % Kc) return fail(what, FTMI_ERR_UNSUPPORTED, "C pt ph pw must divide 2048 (a workgroup's 2048 elements are whole tokens)");
    l.B = g.B; l.C = g.C; l.Cx = g.Cx; l.F = g.F; l.H = g.H; l.W = g.W; l.pt = g.pt; l.ph = g.ph; l.pw = g.pw;
    l.sc = (long)g.F * g.H * g.W; l.sf = (long)g.H * g.W;
    l.Kp = g.Kp; l.copies = g.copies; l.P = g.P; l.drop = 0;
    return lay_derive(l, what);
}

int cog_lay(const ftmi_cog_sample_geometry& g, const char* what, Lay& l) {
    if (g.B <= 0 || g.C <= 0 || g.F <= 0 || g.H <= 0 || g.W <= 0 || g.p <= 0 || g.pt <= 0) return fail(what, FTMI_ERR_INVALID, "extents must be positive");
    if (g.P != 1 && g.P != 2) return fail(what, FTMI_ERR_INVALID, "P is 2 with guidance, 1 without");
    if (g.pt > 2) return fail(what, FTMI_ERR_UNSUPPORTED, "patch_size_t is 1 or 2");
    if (g.F % g.pt || g.H % g.p || g.W % g.p) return fail(what, FTMI_ERR_UNSUPPORTED, "the latent size must be whole patches");
    if (g.drop < 0 || g.drop >= g.pt) return fail(what, FTMI_ERR_INVALID, "drop counts the padded leading frames: 0 <= drop < patch_size_t");
    const long Kc = (long)g.C * g.pt * g.p * g.p;
    if (Kc > 2048 || g.W > 8192) return fail(what, FTMI_ERR_UNSUPPORTED, "patch or row too wide");
    if (Kc % 8) return fail(what, FTMI_ERR_UNSUPPORTED, "C pt p p must be a multiple of 8 (16-byte vectors)");
    l.B = g.B; l.C = g.C; l.Cx = 0; l.F = g.F; l.H = g.H; l.W = g.W; l.pt = g.pt; l.ph = l.pw = g.p;
    l.sc = (long)g.H * g.W; l.sf = (long)g.C * g.H * g.W;
    l.Kp = (int)Kc; l.copies = 1; l.P = g.P; l.drop = g.drop;
    return lay_derive(l, what);
}

int hy_lay(const ftmi_hy_sample_geometry& g, const char* what, Lay& l) {
    if (g.B <= 0 || g.C <= 0 || g.F <= 0 || g.H <= 0 || g.W <= 0 || g.p <= 0 || g.pt <= 0) return fail(what, FTMI_ERR_INVALID, "extents must be positive");
    if (g.P != 1 && g.P != 2) return fail(what, FTMI_ERR_INVALID, "P is 2 with true CFG, 1 without");
    if (g.F % g.pt || g.H % g.p || g.W % g.p) return fail(what, FTMI_ERR_UNSUPPORTED, "the latent size must be whole patches");
    const long Kc = (long)g.C * g.pt * g.p * g.p;
    if (Kc > 2048 || g.W > 8192) return fail(what, FTMI_ERR_UNSUPPORTED, "patch or row too wide");
    if (Kc % 8) return fail(what, FTMI_ERR_UNSUPPORTED, "C pt p p must be a multiple of 8 (16-byte vectors)");
    l.B = g.B; l.C = g.C; l.Cx = 0; l.F = g.F; l.H = g.H; l.W = g.W; l.pt = g.pt; l.ph = l.pw = g.p;
    l.sc = (long)g.F * g.H * g.W; l.sf = (long)g.H * g.W;
    l.Kp = (int)Kc; l.copies = 1; l.P = g.P; l.drop = 0;
    return lay_derive(l, what);
}

int launch_init(const Lay& l, const char* what, const float* latents, const bf16_t* extra, float* x, bf16_t* cols, hipStream_t st) {
    if (misaligned(latents) || misaligned(extra) || misaligned(x) || misaligned(cols)) return fail(what, FTMI_ERR_INVALID, "tensors must be 16-byte aligned");
    size_t lds;
    FTMI_TRY(launch_limits(l, true, what, lds));
    hipLaunchKernelGGL(sample_init_kernel, dim3((unsigned)(l.B * l.fpn * l.hpn)), dim3(256), lds, st, l, latents, extra, x, cols);
    return check_launch(what);
}

template <class Affine>
int launch_finish(const Lay& l, const char* what, const float* x, Affine affine, bf16_t* latents, hipStream_t st) {
    if (misaligned(x) || misaligned(latents)) return fail(what, FTMI_ERR_INVALID, "tensors must be 16-byte aligned");
    size_t lds;
    FTMI_TRY(launch_limits(l, false, what, lds));
    hipLaunchKernelGGL(sample_finish_kernel<Affine>, dim3((unsigned)(l.B * l.fpn * l.hpn)), dim3(256), lds, st, l, x, affine, latents);
    return check_launch(what);
}

}  // namespace

int wan_sample_init(const ftmi_wan_sample_geometry& g, const float* latents, const bf16_t* extra, float* x, bf16_t* cols, hipStream_t st) {
    Lay l;
    FTMI_TRY(wan_lay(g, "wan_sample_init", l));
    if ((g.Cx > 0) != (extra != nullptr)) return set_error(FTMI_ERR_INVALID, "wan_sample_init: the extra channels go with their tensor, and only with it");
    return launch_init(l, "wan_sample_init", latents, extra, x, cols, st);
}

int wan_sample_step(const ftmi_wan_sample_geometry& g, const bf16_t* pred, float* x, const float* sigma, const float* sigma_next, long sig_stride, float guidance,
                    bf16_t* cols, hipStream_t st) {
    Lay l;
    FTMI_TRY(wan_lay(g, "wan_sample_step", l));
    if (pred && (guidance != 1.0f) != (g.P == 2)) return set_error(FTMI_ERR_INVALID, "wan_sample_step: P is 2 with guidance != 1 and 1 with guidance == 1");
    if (pred && (!sigma || !sigma_next)) return set_error(FTMI_ERR_INVALID, "wan_sample_step: sigma / sigma_next missing");
    if (misaligned(pred) || misaligned(x) || misaligned(cols)) return set_error(FTMI_ERR_INVALID, "wan_sample_step: tensors must be 16-byte aligned");
    const long n8 = (long)g.B * l.S * l.Kc / 8, blocks = (n8 + 255) / 256;  // blocks fits an int: lay_derive bounds P B S ld / 8 >= n8
    if (g.P == 2)
        hipLaunchKernelGGL((wan_sample_step_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, l, pred, x, sigma, sigma_next, sig_stride, guidance, cols, n8);
    else
        hipLaunchKernelGGL((wan_sample_step_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, l, pred, x, sigma, sigma_next, sig_stride, guidance, cols, n8);
    return check_launch("wan_sample_step");
}

int wan_sample_step_unipc(const ftmi_wan_sample_geometry& g, const bf16_t* pred, float* x, float* last, const float* m1, float* m2, const float* coef_row,
                          const float* sigma, float guidance, bf16_t* cols, hipStream_t st) {
    Lay l;
    FTMI_TRY(wan_lay(g, "wan_sample_step_unipc", l));
    if (!pred || !last || !m1 || !m2 || !coef_row || !sigma) return set_error(FTMI_ERR_INVALID, "wan_sample_step_unipc: pred, the history buffers, the coefficient row or sigma missing");
    if ((guidance != 1.0f) != (g.P == 2)) return set_error(FTMI_ERR_INVALID, "wan_sample_step_unipc: P is 2 with guidance != 1 and 1 with guidance == 1");
    if (misaligned(pred) || misaligned(x) || misaligned(last) || misaligned(m1) || misaligned(m2) || misaligned(cols))
        return set_error(FTMI_ERR_INVALID, "wan_sample_step_unipc: tensors must be 16-byte aligned");
    if (x == last || x == m1 || x == m2 || last == m1 || last == m2 || m1 == m2) return set_error(FTMI_ERR_INVALID, "wan_sample_step_unipc: x, last, m1 and m2 are four buffers");
    const long n8 = (long)g.B * l.S * l.Kc / 8, blocks = (n8 + 255) / 256;  // blocks fits an int: lay_derive bounds P B S ld / 8 >= n8
    if (g.P == 2)
        hipLaunchKernelGGL((wan_sample_step_unipc_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, l, pred, x, last, m1, m2, coef_row, sigma, guidance, cols, n8);
    else
        hipLaunchKernelGGL((wan_sample_step_unipc_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, l, pred, x, last, m1, m2, coef_row, sigma, guidance, cols, n8);
    return check_launch("wan_sample_step_unipc");
}

int wan_sample_finish(const ftmi_wan_sample_geometry& g, const float* x, const float* mean, const float* std_, bf16_t* latents, hipStream_t st) {
    Lay l;
    FTMI_TRY(wan_lay(g, "wan_sample_finish", l));
    return launch_finish(l, "wan_sample_finish", x, ChannelAffine{mean, std_}, latents, st);
}

int cog_sample_init(const ftmi_cog_sample_geometry& g, const float* latents, float* x, bf16_t* cols, hipStream_t st) {
    Lay l;
    FTMI_TRY(cog_lay(g, "cog_sample_init", l));
    return launch_init(l, "cog_sample_init", latents, nullptr, x, cols, st);
}

int cog_sample_step(const ftmi_cog_sample_geometry& g, const bf16_t* pred, float* x, const float* coef, int step, float guidance, bf16_t* cols, hipStream_t st) {
    Lay l;
    FTMI_TRY(cog_lay(g, "cog_sample_step", l));
    if (pred && (guidance != 1.0f) != (g.P == 2)) return set_error(FTMI_ERR_INVALID, "cog_sample_step: P is 2 with guidance != 1 and 1 with guidance == 1");
    if (pred && (!coef || step < 0)) return set_error(FTMI_ERR_INVALID, "cog_sample_step: the coefficient table or the step index is missing");
    if (misaligned(pred) || misaligned(x) || misaligned(cols)) return set_error(FTMI_ERR_INVALID, "cog_sample_step: tensors must be 16-byte aligned");
    const long n8 = (long)g.B * l.S * l.Kc / 8, blocks = (n8 + 255) / 256;
    if (g.P == 2)
        hipLaunchKernelGGL((cog_sample_step_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, pred, x, coef, step, guidance, cols, n8);
    else
        hipLaunchKernelGGL((cog_sample_step_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, pred, x, coef, step, guidance, cols, n8);
    return check_launch("cog_sample_step");
}

int cog_sample_step_dpm(const ftmi_cog_sample_geometry& g, const bf16_t* pred, float* x, float* old, const float* noise, const float* coef_row, bf16_t* cols,
                        hipStream_t st) {
    Lay l;
    FTMI_TRY(cog_lay(g, "cog_sample_step_dpm", l));
    if (!pred || !x || !old || !coef_row) return set_error(FTMI_ERR_INVALID, "cog_sample_step_dpm: pred, x, old or the coefficient row missing");
    if (misaligned(pred) || misaligned(x) || misaligned(old) || misaligned(noise) || misaligned(cols))
        return set_error(FTMI_ERR_INVALID, "cog_sample_step_dpm: tensors must be 16-byte aligned");
    if (x == old || x == noise || old == noise) return set_error(FTMI_ERR_INVALID, "cog_sample_step_dpm: x, old and noise are three buffers");
    const long n8 = (long)g.B * l.S * l.Kc / 8, blocks = (n8 + 255) / 256;
    if (g.P == 2)
        hipLaunchKernelGGL((cog_sample_step_dpm_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, pred, x, old, noise, coef_row, cols, n8);
    else
        hipLaunchKernelGGL((cog_sample_step_dpm_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, pred, x, old, noise, coef_row, cols, n8);
    return check_launch("cog_sample_step_dpm");
}

int cog_sample_pack(const ftmi_cog_sample_geometry& g, const float* latents, int n, float* out, hipStream_t st) {
    if (n <= 0 || g.B <= 0 || (long)n * g.B > 0x7fffffffL) return set_error(FTMI_ERR_INVALID, "cog_sample_pack: n and B must be positive (and n B fit an int)");
    ftmi_cog_sample_geometry gn = g;
    gn.B = n * g.B;  // n tensors of B samples are n B samples to the index map
    Lay l;
    FTMI_TRY(cog_lay(gn, "cog_sample_pack", l));
    if ((long)l.B * l.S * l.Kc / 8 > 0x7fffffffL * 256L) return fail("cog_sample_pack", FTMI_ERR_UNSUPPORTED, "too many elements for one launch");
    l.P = 0;  // no row group of cols is written
    return launch_init(l, "cog_sample_pack", latents, nullptr, out, nullptr, st);
}

int cog_sample_finish(const ftmi_cog_sample_geometry& g, const float* x, float k, bf16_t* latents, hipStream_t st) {
    Lay l;
    FTMI_TRY(cog_lay(g, "cog_sample_finish", l));
    return launch_finish(l, "cog_sample_finish", x, ScalarAffine{k}, latents, st);
}

int hy_sample_init(const ftmi_hy_sample_geometry& g, const float* latents, float* x, bf16_t* cols, hipStream_t st) {
    Lay l;
    FTMI_TRY(hy_lay(g, "hy_sample_init", l));
    return launch_init(l, "hy_sample_init", latents, nullptr, x, cols, st);
}

int hy_sample_step(const ftmi_hy_sample_geometry& g, const bf16_t* pred, float* x, const float* sigmas, int step, float true_cfg, bf16_t* cols, hipStream_t st) {
    Lay l;
    FTMI_TRY(hy_lay(g, "hy_sample_step", l));
    if (pred && (true_cfg != 1.0f) != (g.P == 2)) return set_error(FTMI_ERR_INVALID, "hy_sample_step: P is 2 with true_cfg != 1 and 1 with true_cfg == 1");
    if (pred && (!sigmas || step < 0)) return set_error(FTMI_ERR_INVALID, "hy_sample_step: the sigma table or the step index is missing");
    if (misaligned(pred) || misaligned(x) || misaligned(cols)) return set_error(FTMI_ERR_INVALID, "hy_sample_step: tensors must be 16-byte aligned");
    const long n8 = (long)g.B * l.S * l.Kc / 8, blocks = (n8 + 255) / 256;
    if (g.P == 2)
        hipLaunchKernelGGL((hy_sample_step_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, pred, x, sigmas, step, true_cfg, cols, n8);
    else
        hipLaunchKernelGGL((hy_sample_step_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, pred, x, sigmas, step, true_cfg, cols, n8);
    return check_launch("hy_sample_step");
}

int hy_sample_finish(const ftmi_hy_sample_geometry& g, const float* x, float k, bf16_t* latents, hipStream_t st) {
    Lay l;
    FTMI_TRY(hy_lay(g, "hy_sample_finish", l));
    return launch_finish(l, "hy_sample_finish", x, ScalarAffine{k}, latents, st);
}

int wan_sample_mod(const bf16_t* const* tables, int L, const bf16_t* tproj, float* mod, int rows, int D, hipStream_t st) {
    if (L <= 0 || rows <= 0 || D <= 0) return set_error(FTMI_ERR_INVALID, "wan_sample_mod: empty problem");
    if (L > kModMaxBlocks) return set_error(FTMI_ERR_UNSUPPORTED, "wan_sample_mod: at most 40 blocks per launch");
    if ((6 * D) % 8) return set_error(FTMI_ERR_UNSUPPORTED, "wan_sample_mod: 6 D must be a multiple of 8 (16-byte vectors)");
    ModArgs a;
    for (int l = 0; l < L; ++l) {
        if (!tables[l] || misaligned(tables[l])) return set_error(FTMI_ERR_INVALID, "wan_sample_mod: every scale_shift_table must be a 16-byte aligned pointer");
        a.table[l] = tables[l];
    }
    for (int l = L; l < kModMaxBlocks; ++l) a.table[l] = nullptr;
    if (misaligned(tproj) || misaligned(mod)) return set_error(FTMI_ERR_INVALID, "wan_sample_mod: tensors must be 16-byte aligned");
    a.tproj = tproj; a.out = mod; a.rows = rows; a.n8 = 6 * D / 8;
    hipLaunchKernelGGL(wan_sample_mod_kernel, dim3((a.n8 + 255) / 256, L), dim3(256), 0, st, a);
    return check_launch("wan_sample_mod");
}

}  // namespace ftmi
