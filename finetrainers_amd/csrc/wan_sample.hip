// Wan latent sampling, the kernels around the DiT forward of a denoising loop (the orchestrator is wan_sample in wan_sample_dit.hip).
//
// The sampler state lives in the patch embedding's OPERAND layout, so a step needs no patchify / un-patchify:
//   state  x     fp32 [B, S, Kc]       Kc = C pt ph pw columns in the patch embedding's order (c, pt, ph, pw), tokens in (f, h, w) order
//   input  cols  bf16 [P B S, ld]      the patch-embedding GEMM's operand.  ld = copies Kp: Kp the stored patch width (64 T2V, 192 I2V with 144 used, 128 control),
//                                      copies = 2 for a model with the folded patch adapter ([cols | cols], what ftmi_wan_control_pack writes).  Columns [0, Kc) of
//                                      every copy are bf16(x); the others (I2V: mask + condition, control: control latents, padding: +0) are constant over the loop.
//                                      P = 2 row groups with guidance (rows [0, B S) unconditional, [B S, 2 B S) conditional), 1 without.
//   output pred  bf16 [P B, S, po]     what proj_out writes, po = Kc, columns in (pt, ph, pw, c) order -- NOT the input order.
//
// wan_sample_init: latents fp32 [B, C, F, H, W] (+ extra bf16 [B, Cx, F, H, W]) -> x (exact) and every row group and copy of cols.  One workgroup per row of
//   patches (b, f', h'): the pt ph W-element runs of every channel are staged in the LDS through the 16-byte vectors that cover them, then every thread gathers
//   8 columns of one token and stores them as vectors.  Bytes moved per state element: 4 read, 4 + 2 P copies written; per extra element 2 read, 2 P copies written.
// wan_sample_step: classifier-free-guidance combine + flow-match Euler update of one step, one pass:
//       d = c - u;   v = fma(g, d, u);   dt = sigma_next - sigma;   x <- fma(dt, v, x)            (guidance == 1: v = c, no unconditional half)
//   all fp32, and bf16(x) (round to nearest even) goes to columns [0, Kc) of every row group and copy of cols.  A thread reads 16 bytes of each half of pred,
//   combines them in pred's order, and hands v to the thread that owns the state columns through the LDS: state column c pv + p is pred column p C + c
//   (pv = pt ph pw), so a token's 128 bytes are permuted on chip and every global access stays a 16-byte vector.  sigma / sigma_next are read from the device.
//   pred == nullptr: no update, only the copies.  The arithmetic is cfg_euler_step's (ltx_sample.hip), which restates [upstream, unpinned]
//   FlowMatchEulerDiscreteScheduler.step after the pipeline's noise_uncond + guidance_scale * (noise_pred - noise_uncond); the state is kept in fp32.
//   Bytes moved per element of x: 12 + 2 P copies with guidance (read u 2 + c 2 + x 4, write x 4 + cols): 16 for T2V / I2V, 20 with the folded patch adapter;
//   10 + 2 copies without guidance: 12 / 14.
// wan_sample_finish: x fp32 [B, S, Kc] -> latents bf16 [B, C, F, H, W] = bf16(x * std[c] + mean[c]).  std is the VAE's REAL standard deviation -- not the
//   1 / std the training processors hand over (finetrainers/models/wan/base_specification.py multiplies by latents_std = 1 / std when it normalises).  The
//   transpose goes through LDS tiles as in unpack_denorm_kernel: 16-byte reads along the token columns, 16-byte writes along W when the runs are 16-byte
//   aligned (ph W % 8 == 0), element stores otherwise; the 2 C statistics are scalar loads.  Bytes moved per element: 4 read + 2 written.
// wan_sample_mod: the fp32 modulation of all L blocks for ONE step, mod [L, rows, 6, D] = float(scale_shift_table_l) + float(tproj_step) (the expression of
//   finetrainers_amd/wan/block.py _fwd), every row of a step sharing one timestep: there is no [steps, L, ...] table.  Bytes per output element: 4 written, 4 / rows read.
#include "common.hip.h"
#include "kernels.h"

namespace ftmi {

namespace {

FTMI_DEVICE void unpack8(const u32x4& p, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(p[i] << 16);
        f[2 * i + 1] = __uint_as_float(p[i] & 0xffff0000u);
    }
}

// what the three layout kernels share, derived once on the host
struct Lay {
    int B, C, Cx, F, H, W, pt, ph, pw;
    int pv, Kc, Kx, Kp, ld, P, copies;
    int fpn, hpn, wpn;  // patches along F, H, W
    long S;             // tokens per sample
    int seg_len;        // ph W: one contiguous run of a channel inside a row of patches
    int pitch_f, pitch_h;  // LDS elements per run: fp32 (multiple of 4) / bf16 (multiple of 8)
};

// state column k -> (run = c pt + dt, offset inside the run for token w of the row of patches)
FTMI_DEVICE void col_src(const Lay& g, int k, int w, int& run, int& off) {
    const int c = k / g.pv, rem = k - c * g.pv;
    const int dt = rem / (g.ph * g.pw), dy = (rem / g.pw) % g.ph, dx = rem % g.pw;
    run = c * g.pt + dt;
    off = dy * g.W + w * g.pw + dx;
}

FTMI_DEVICE void block_coords(const Lay& g, int& b, int& fp, int& hp) {
    int t = blockIdx.x;
    hp = t % g.hpn; t /= g.hpn;
    fp = t % g.fpn;
    b = t / g.fpn;
}

// grid B f' h' workgroups of 256; dynamic LDS: C pt pitch_f floats, then Cx pt pitch_h bf16
__global__ __launch_bounds__(256) void wan_sample_init_kernel(Lay g, const float* __restrict__ lat, const bf16_t* __restrict__ extra, float* __restrict__ x,
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
            const int c = run / g.pt, dt = run - c * g.pt;
            const long start = ((((long)b * g.C + c) * g.F + fp * g.pt + dt) * g.H + (long)hp * g.ph) * g.W;
            const long gv = (start >> 2) + vi;
            if (gv < ((start + g.seg_len + 3) >> 2)) reinterpret_cast<f32x4*>(lf)[idx] = reinterpret_cast<const f32x4*>(lat)[gv];
        }
    }
    if (g.Cx > 0) {
        const int nrun = g.Cx * g.pt, vpr = g.pitch_h / 8;
        for (int idx = tid; idx < nrun * vpr; idx += 256) {
            const int run = idx / vpr, vi = idx - run * vpr;
            const int c = run / g.pt, dt = run - c * g.pt;
            const long start = ((((long)b * g.Cx + c) * g.F + fp * g.pt + dt) * g.H + (long)hp * g.ph) * g.W;
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
                const int c = run / g.pt, dt = run - c * g.pt;
                const long start = ((((long)b * g.C + c) * g.F + fp * g.pt + dt) * g.H + (long)hp * g.ph) * g.W;
                v[e] = lf[run * g.pitch_f + (int)(start & 3) + off];
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
                const int c = run / g.pt, dt = run - c * g.pt;
                const long start = ((((long)b * g.Cx + c) * g.F + fp * g.pt + dt) * g.H + (long)hp * g.ph) * g.W;
                h[e] = lh[run * g.pitch_h + (int)(start & 7) + off];
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
            const u32x4* pp = reinterpret_cast<const u32x4*>(pred);
            if (kCfg) {
                float u[8], c[8];
                unpack8(pp[i], u);
                unpack8(pp[n8 + i], c);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaf(gd, c[e] - u[e], u[e]);
            } else {
                unpack8(pp[i], v);
            }
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
    if (cols) {
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack2bf(xv[2 * e], xv[2 * e + 1]);
#pragma unroll
        for (int p = 0; p < (kCfg ? 2 : 1); ++p)
            for (int cp = 0; cp < g.copies; ++cp)
                *reinterpret_cast<u32x4*>(cols + (((long)p * g.B + b) * g.S + t) * g.ld + (long)cp * g.Kp + j0) = o;
    }
}

// grid B f' h' workgroups of 256; dynamic LDS: C pt pitch_h bf16, [run][dy W + w pw + dx]
__global__ __launch_bounds__(256) void wan_sample_finish_kernel(Lay g, const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ std_,
                                                                bf16_t* __restrict__ out) {
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
            const int c = (k0 + e) / g.pv;
            lh[run * g.pitch_h + off] = f2bf(v[e] * std_[c] + mean[c]);
        }
    }
    __syncthreads();
    const int nrun = g.C * g.pt;
    auto run_start = [&](int run) {
        const int c = run / g.pt, dt = run - c * g.pt;
        return ((((long)b * g.C + c) * g.F + fp * g.pt + dt) * g.H + (long)hp * g.ph) * g.W;
    };
    if ((g.seg_len & 7) == 0) {  // every run starts and ends on a 16-byte boundary
        const int vpr = g.seg_len / 8;
        for (int idx = tid; idx < nrun * vpr; idx += 256) {
            const int run = idx / vpr, vi = idx - run * vpr;
            *reinterpret_cast<u32x4*>(out + run_start(run) + vi * 8) = *reinterpret_cast<const u32x4*>(lh + run * g.pitch_h + vi * 8);
        }
    } else {  // the runs are not 16-byte aligned: element stores
        for (int idx = tid; idx < nrun * g.seg_len; idx += 256) {
            const int run = idx / g.seg_len, e = idx - run * g.seg_len;
            out[run_start(run) + e] = lh[run * g.pitch_h + e];
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

// Checks the geometry and derives the kernels' layout.
int make_lay(const ftmi_wan_sample_geometry& g, const char* what, Lay& l) {
    char msg[200];
    auto fail = [&](int code, const char* why) {
        snprintf(msg, sizeof(msg), "%s: %s", what, why);
        return set_error(code, msg);
    };
    if (g.B <= 0 || g.C <= 0 || g.Cx < 0 || g.F <= 0 || g.H <= 0 || g.W <= 0 || g.pt <= 0 || g.ph <= 0 || g.pw <= 0 || g.Kp <= 0)
        return fail(FTMI_ERR_INVALID, "extents must be positive");
    if (g.copies != 1 && g.copies != 2) return fail(FTMI_ERR_INVALID, "copies is 1, or 2 for [cols | cols]");
    if (g.P != 1 && g.P != 2) return fail(FTMI_ERR_INVALID, "P is 2 with guidance, 1 without");
    if (g.F % g.pt || g.H % g.ph || g.W % g.pw) return fail(FTMI_ERR_UNSUPPORTED, "the latent size must be whole patches");
    const long pv = (long)g.pt * g.ph * g.pw, Kc = g.C * pv, Kx = g.Cx * pv, ld = (long)g.copies * g.Kp;
    if (Kc > 2048 || Kx > 65536 || g.Kp > 65536) return fail(FTMI_ERR_UNSUPPORTED, "patch too wide");
    if (Kc % 8 || Kx % 8) return fail(FTMI_ERR_UNSUPPORTED, "C pt ph pw (and the extra channels' columns) must be multiples of 8 (16-byte vectors)");
    if (g.Kp % 8 || ld % 8) return fail(FTMI_ERR_UNSUPPORTED, "the row stride ld must be a multiple of 8 (16-byte vectors)");
    if (Kc != g.po) return fail(FTMI_ERR_INVALID, "C pt ph pw must equal po, the width of proj_out");
    if (Kc + Kx > g.Kp) return fail(FTMI_ERR_INVALID, "the state and extra columns do not fit the stored patch width Kp");
    if (2048 % Kc) return fail(FTMI_ERR_UNSUPPORTED, "C pt ph pw must divide 2048 (a workgroup's 2048 elements are whole tokens)");
    l.B = g.B; l.C = g.C; l.Cx = g.Cx; l.F = g.F; l.H = g.H; l.W = g.W; l.pt = g.pt; l.ph = g.ph; l.pw = g.pw;
    l.pv = (int)pv; l.Kc = (int)Kc; l.Kx = (int)Kx; l.Kp = g.Kp; l.ld = (int)ld; l.P = g.P; l.copies = g.copies;
    l.fpn = g.F / g.pt; l.hpn = g.H / g.ph; l.wpn = g.W / g.pw;
    l.S = (long)l.fpn * l.hpn * l.wpn;
    l.seg_len = g.ph * g.W;
    l.pitch_f = 4 * ((l.seg_len + 3) / 4 + 1);
    l.pitch_h = 8 * ((l.seg_len + 7) / 8 + 1);
    if ((long)g.B * l.fpn * l.hpn > 0x7fffffffL || (long)g.P * g.B * l.S * ld / 8 > 0x7fffffffL * 256L) return fail(FTMI_ERR_UNSUPPORTED, "too many elements for one launch");
    return 0;
}

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

int wan_sample_init(const ftmi_wan_sample_geometry& g, const float* latents, const bf16_t* extra, float* x, bf16_t* cols, hipStream_t st) {
    Lay l;
    FTMI_TRY(make_lay(g, "wan_sample_init", l));
    if ((g.Cx > 0) != (extra != nullptr)) return set_error(FTMI_ERR_INVALID, "wan_sample_init: the extra channels go with their tensor, and only with it");
    if (misaligned(latents) || misaligned(extra) || misaligned(x) || misaligned(cols)) return set_error(FTMI_ERR_INVALID, "wan_sample_init: tensors must be 16-byte aligned");
    const long per = (long)g.F * g.H * g.W;
    if (((long)g.B * g.C * per) % 4 || ((long)g.B * g.Cx * per) % 8)
        return set_error(FTMI_ERR_UNSUPPORTED, "wan_sample_init: the latents must be a whole number of 16-byte vectors");
    const size_t lds = (size_t)g.C * g.pt * l.pitch_f * 4 + (size_t)g.Cx * g.pt * l.pitch_h * 2;
    if (lds > 64 * 1024) return set_error(FTMI_ERR_UNSUPPORTED, "wan_sample_init: a row of patches does not fit the LDS");
    hipLaunchKernelGGL(wan_sample_init_kernel, dim3((unsigned)(g.B * l.fpn * l.hpn)), dim3(256), lds, st, l, latents, extra, x, cols);
    return check_launch("wan_sample_init");
}

int wan_sample_step(const ftmi_wan_sample_geometry& g, const bf16_t* pred, float* x, const float* sigma, const float* sigma_next, long sig_stride, float guidance,
                    bf16_t* cols, hipStream_t st) {
    Lay l;
    FTMI_TRY(make_lay(g, "wan_sample_step", l));
    if (pred && (guidance != 1.0f) != (g.P == 2)) return set_error(FTMI_ERR_INVALID, "wan_sample_step: P is 2 with guidance != 1 and 1 with guidance == 1");
    if (pred && (!sigma || !sigma_next)) return set_error(FTMI_ERR_INVALID, "wan_sample_step: sigma / sigma_next missing");
    if (misaligned(pred) || misaligned(x) || misaligned(cols)) return set_error(FTMI_ERR_INVALID, "wan_sample_step: tensors must be 16-byte aligned");
    const long n8 = (long)g.B * l.S * l.Kc / 8, blocks = (n8 + 255) / 256;
    if (blocks > 0x7fffffffL) return set_error(FTMI_ERR_UNSUPPORTED, "wan_sample_step: too many elements for one launch");
    if (g.P == 2)
        hipLaunchKernelGGL((wan_sample_step_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, l, pred, x, sigma, sigma_next, sig_stride, guidance, cols, n8);
    else
        hipLaunchKernelGGL((wan_sample_step_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, l, pred, x, sigma, sigma_next, sig_stride, guidance, cols, n8);
    return check_launch("wan_sample_step");
}

int wan_sample_finish(const ftmi_wan_sample_geometry& g, const float* x, const float* mean, const float* std_, bf16_t* latents, hipStream_t st) {
    Lay l;
    FTMI_TRY(make_lay(g, "wan_sample_finish", l));
    if (misaligned(x) || misaligned(latents)) return set_error(FTMI_ERR_INVALID, "wan_sample_finish: tensors must be 16-byte aligned");
    const size_t lds = (size_t)g.C * g.pt * l.pitch_h * 2;
    if (lds > 64 * 1024) return set_error(FTMI_ERR_UNSUPPORTED, "wan_sample_finish: a row of patches does not fit the LDS");
    hipLaunchKernelGGL(wan_sample_finish_kernel, dim3((unsigned)(g.B * l.fpn * l.hpn)), dim3(256), lds, st, l, x, mean, std_, latents);
    return check_launch("wan_sample_finish");
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
