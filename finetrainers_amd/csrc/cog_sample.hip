// CogVideoX latent sampling, the kernels around the DiT forward of a denoising loop (the orchestrator is cog_sample in cog_dit.hip, next to the block walk).
//
// CogVideoX's patch embedding reads its operand in (c, ph, pw) order -- (c, pt, ph, pw) with patch_size_t -- and proj_out writes the SAME column order
// (tests/test_gpu_cogvideox.py::test_patchify_roundtrip_and_position_table pins both), so the sampler state lives in that layout and a step permutes nothing:
//   state  x     fp32 [B, S, Kc]       Kc = C pt p p columns, column ((c pt + dt) p + dy) p + dx; S = (F / pt)(H / p)(W / p) tokens in (f, h, w) order
//   input  cols  bf16 [P B S, Kc]      the patch-embedding GEMM's operand: bf16(x) in every row group.  P = 2 with guidance (rows [0, B S) unconditional,
//                                      [B S, 2 B S) conditional), 1 without.
//   output pred  bf16 [P B, S, Kc]     what proj_out writes, the same columns.
// The latents are [B, F, C, H, W] (frames BEFORE channels, the CogVideoX convention), so the contiguous piece of a channel inside a row of patches is the
// run of p W elements of one (frame, channel) plane.
//
// cog_sample_init: noise fp32 [B, F, C, H, W] -> x (exact) and every row group of cols.  One workgroup per row of patches (b, f', h'): the C pt runs are staged
//   in the LDS through the aligned 16-byte vectors that cover them, then every thread gathers 8 columns of one token and stores them as vectors.
//   Bytes moved per state element: 4 read, 4 + 2 P written.
// cog_sample_step: classifier-free-guidance combine + DDIM update (v-prediction, eta = 0) of one step, one row-major pass:
//       d = c - u;   v = fma(g, d, u);   x <- fma(cx, x, cv * v)                                   (guidance == 1: v = c, no unconditional half)
//   all fp32, and bf16(x) (round to nearest even) goes to every row group of cols.  (cx, cv) are the step's two numbers of the host-folded scheduler
//   ([upstream, unpinned] CogVideoXDDIMScheduler.step is linear in (x, v): finetrainers_amd/cogvideox/sampler.py cog_ddim_tables), read from a device table.
//   A thread owns 8 consecutive elements; the grid is sized from the element count and the last workgroup's tail is masked.  pred == nullptr: only the copies.
//   Bytes moved per element of x: 12 + 2 P with guidance (read u 2 + c 2 + x 4, write x 4 + cols 4) = 16; 10 + 2 = 12 without.
// cog_sample_finish: x fp32 [B, S, Kc] -> latents bf16 [B, F - drop, C, H, W] = bf16(x * k), the inverse permutation of init; the first `drop` frames (what the
//   pipeline pads at the front for patch_size_t and discards after the loop) are not written.  16-byte reads along the token columns, 16-byte writes along the
//   runs when they are 16-byte aligned (p W % 8 == 0), element stores otherwise.  Bytes moved per element: 4 read + 2 written.
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

// what the layout kernels share, derived once on the host
struct Lay {
    int B, C, F, H, W, p, pt, P, drop;
    int pp, Kc;         // p p, C pt p p
    int fpn, hpn, wpn;  // patches along F, H, W
    long S;             // tokens per sample
    int seg_len;        // p W: one contiguous run of a (frame, channel) plane inside a row of patches
    int pitch_f, pitch_h;  // LDS elements per run: fp32 (multiple of 4) / bf16 (multiple of 8)
};

// state column k -> (run = c pt + dt, offset inside the run for token w of the row of patches)
FTMI_DEVICE void col_src(const Lay& g, int k, int w, int& run, int& off) {
    run = k / g.pp;
    const int rem = k - run * g.pp;
    const int dy = rem / g.p, dx = rem - dy * g.p;
    off = dy * g.W + w * g.p + dx;
}

// first element of run (c, dt) of the row of patches (b, f', h') in a tensor [B, frames, C, H, W] whose frame 0 is frame `first` of the grid
FTMI_DEVICE long run_start(const Lay& g, int b, int fp, int hp, int run, int frames, int first) {
    const int c = run / g.pt, dt = run - c * g.pt;
    return ((((long)b * frames + (fp * g.pt + dt - first)) * g.C + c) * g.H + (long)hp * g.p) * g.W;
}

FTMI_DEVICE void block_coords(const Lay& g, int& b, int& fp, int& hp) {
    int t = blockIdx.x;
    hp = t % g.hpn; t /= g.hpn;
    fp = t % g.fpn;
    b = t / g.fpn;
}

// grid B f' h' workgroups of 256; dynamic LDS: C pt pitch_f floats
__global__ __launch_bounds__(256) void cog_sample_init_kernel(Lay g, const float* __restrict__ lat, float* __restrict__ x, bf16_t* __restrict__ cols) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lf = reinterpret_cast<float*>(smem);
    int b, fp, hp;
    block_coords(g, b, fp, hp);
    const int tid = threadIdx.x;
    {  // the runs, through the aligned 16-byte vectors that cover them (the tensor is a whole number of vectors: the cover stays inside it)
        const int nrun = g.C * g.pt, vpr = g.pitch_f / 4;
        for (int idx = tid; idx < nrun * vpr; idx += 256) {
            const int run = idx / vpr, vi = idx - run * vpr;
            const long start = run_start(g, b, fp, hp, run, g.F, 0);
            const long gv = (start >> 2) + vi;
            if (gv < ((start + g.seg_len + 3) >> 2)) reinterpret_cast<f32x4*>(lf)[idx] = reinterpret_cast<const f32x4*>(lat)[gv];
        }
    }
    __syncthreads();
    // out: wpn tokens x Kc / 8 vectors of 8 columns; element e of a run sits (start mod vector) + e into its LDS slot
    const int vpt = g.Kc / 8;
    const long n = (long)g.B * g.S * g.Kc;
    for (int idx = tid; idx < g.wpn * vpt; idx += 256) {
        const int w = idx / vpt, k0 = (idx - w * vpt) * 8;
        const long t = ((long)fp * g.hpn + hp) * g.wpn + w;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int run, off;
            col_src(g, k0 + e, w, run, off);
            v[e] = lf[run * g.pitch_f + (int)(run_start(g, b, fp, hp, run, g.F, 0) & 3) + off];
        }
        const long at = ((long)b * g.S + t) * g.Kc + k0;
        f32x4* xp = reinterpret_cast<f32x4*>(x + at);
        xp[0] = f32x4{v[0], v[1], v[2], v[3]};
        xp[1] = f32x4{v[4], v[5], v[6], v[7]};
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack2bf(v[2 * e], v[2 * e + 1]);
        for (int p = 0; p < g.P; ++p) *reinterpret_cast<u32x4*>(cols + (long)p * n + at) = o;
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
        const u32x4* pp = reinterpret_cast<const u32x4*>(pred);
        float v[8];
        if (kCfg) {
            float u[8], c[8];
            unpack8(pp[i], u);
            unpack8(pp[n8 + i], c);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaf(gd, c[e] - u[e], u[e]);
        } else {
            unpack8(pp[i], v);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = __builtin_fmaf(cx, xv[e], cv * v[e]);
        xp[0] = f32x4{xv[0], xv[1], xv[2], xv[3]};
        xp[1] = f32x4{xv[4], xv[5], xv[6], xv[7]};
    }
    if (cols) {
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack2bf(xv[2 * e], xv[2 * e + 1]);
        u32x4* cp = reinterpret_cast<u32x4*>(cols);
#pragma unroll
        for (int p = 0; p < (kCfg ? 2 : 1); ++p) cp[(long)p * n8 + i] = o;
    }
}

// grid B f' h' workgroups of 256; dynamic LDS: C pt pitch_h bf16, [run][dy W + w p + dx]
__global__ __launch_bounds__(256) void cog_sample_finish_kernel(Lay g, const float* __restrict__ x, float k, bf16_t* __restrict__ out) {
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
            lh[run * g.pitch_h + off] = f2bf(v[e] * k);
        }
    }
    __syncthreads();
    const int nrun = g.C * g.pt, frames = g.F - g.drop;
    auto kept = [&](int run) { return fp * g.pt + (run % g.pt) >= g.drop; };  // the run's frame is not one of the dropped leading frames
    if ((g.seg_len & 7) == 0) {  // every run starts and ends on a 16-byte boundary
        const int vpr = g.seg_len / 8;
        for (int idx = tid; idx < nrun * vpr; idx += 256) {
            const int run = idx / vpr, vi = idx - run * vpr;
            if (kept(run)) *reinterpret_cast<u32x4*>(out + run_start(g, b, fp, hp, run, frames, g.drop) + vi * 8) = *reinterpret_cast<const u32x4*>(lh + run * g.pitch_h + vi * 8);
        }
    } else {  // the runs are not 16-byte aligned: element stores
        for (int idx = tid; idx < nrun * g.seg_len; idx += 256) {
            const int run = idx / g.seg_len, e = idx - run * g.seg_len;
            if (kept(run)) out[run_start(g, b, fp, hp, run, frames, g.drop) + e] = lh[run * g.pitch_h + e];
        }
    }
}

// Checks the geometry and derives the kernels' layout.
int make_lay(const ftmi_cog_sample_geometry& g, const char* what, Lay& l) {
    char msg[200];
    auto fail = [&](int code, const char* why) {
        snprintf(msg, sizeof(msg), "%s: %s", what, why);
        return set_error(code, msg);
    };
    if (g.B <= 0 || g.C <= 0 || g.F <= 0 || g.H <= 0 || g.W <= 0 || g.p <= 0 || g.pt <= 0) return fail(FTMI_ERR_INVALID, "extents must be positive");
    if (g.P != 1 && g.P != 2) return fail(FTMI_ERR_INVALID, "P is 2 with guidance, 1 without");
    if (g.pt > 2) return fail(FTMI_ERR_UNSUPPORTED, "patch_size_t is 1 or 2");
    if (g.F % g.pt || g.H % g.p || g.W % g.p) return fail(FTMI_ERR_UNSUPPORTED, "the latent size must be whole patches");
    if (g.drop < 0 || g.drop >= g.pt) return fail(FTMI_ERR_INVALID, "drop counts the padded leading frames: 0 <= drop < patch_size_t");
    const long Kc = (long)g.C * g.pt * g.p * g.p;
    if (Kc > 2048 || g.W > 8192) return fail(FTMI_ERR_UNSUPPORTED, "patch or row too wide");
    if (Kc % 8) return fail(FTMI_ERR_UNSUPPORTED, "C pt p p must be a multiple of 8 (16-byte vectors)");
    l.B = g.B; l.C = g.C; l.F = g.F; l.H = g.H; l.W = g.W; l.p = g.p; l.pt = g.pt; l.P = g.P; l.drop = g.drop;
    l.pp = g.p * g.p; l.Kc = (int)Kc;
    l.fpn = g.F / g.pt; l.hpn = g.H / g.p; l.wpn = g.W / g.p;
    l.S = (long)l.fpn * l.hpn * l.wpn;
    l.seg_len = g.p * g.W;
    l.pitch_f = 4 * ((l.seg_len + 3) / 4 + 1);
    l.pitch_h = 8 * ((l.seg_len + 7) / 8 + 1);
    if ((long)g.B * l.fpn * l.hpn > 0x7fffffffL || (long)g.B * l.S * Kc / 8 > 0x7fffffffL * 256L) return fail(FTMI_ERR_UNSUPPORTED, "too many elements for one launch");
    return 0;
}

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

int cog_sample_init(const ftmi_cog_sample_geometry& g, const float* latents, float* x, bf16_t* cols, hipStream_t st) {
    Lay l;
    FTMI_TRY(make_lay(g, "cog_sample_init", l));
    if (misaligned(latents) || misaligned(x) || misaligned(cols)) return set_error(FTMI_ERR_INVALID, "cog_sample_init: tensors must be 16-byte aligned");
    if (((long)g.B * g.F * g.C * g.H * g.W) % 4) return set_error(FTMI_ERR_UNSUPPORTED, "cog_sample_init: the latents must be a whole number of 16-byte vectors");
    const size_t lds = (size_t)g.C * g.pt * l.pitch_f * 4;
    if (lds > 64 * 1024) return set_error(FTMI_ERR_UNSUPPORTED, "cog_sample_init: a row of patches does not fit the LDS");
    hipLaunchKernelGGL(cog_sample_init_kernel, dim3((unsigned)(g.B * l.fpn * l.hpn)), dim3(256), lds, st, l, latents, x, cols);
    return check_launch("cog_sample_init");
}

int cog_sample_step(const ftmi_cog_sample_geometry& g, const bf16_t* pred, float* x, const float* coef, int step, float guidance, bf16_t* cols, hipStream_t st) {
    Lay l;
    FTMI_TRY(make_lay(g, "cog_sample_step", l));
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

int cog_sample_finish(const ftmi_cog_sample_geometry& g, const float* x, float k, bf16_t* latents, hipStream_t st) {
    Lay l;
    FTMI_TRY(make_lay(g, "cog_sample_finish", l));
    if (misaligned(x) || misaligned(latents)) return set_error(FTMI_ERR_INVALID, "cog_sample_finish: tensors must be 16-byte aligned");
    const size_t lds = (size_t)g.C * g.pt * l.pitch_h * 2;
    if (lds > 64 * 1024) return set_error(FTMI_ERR_UNSUPPORTED, "cog_sample_finish: a row of patches does not fit the LDS");
    hipLaunchKernelGGL(cog_sample_finish_kernel, dim3((unsigned)(g.B * l.fpn * l.hpn)), dim3(256), lds, st, l, x, k, latents);
    return check_launch("cog_sample_finish");
}

}  // namespace ftmi
