// Wan control LoRA: what the control recipe adds OUTSIDE the blocks.
//   f32_gemm          c (+)= scale * a b in fp32 FMAs with strided (possibly transposed) operands, optionally also as bf16 [hi | lo] column planes:
//                     the fold dW = s B A of the full-rank patch-embedding adapter and its two gradients grad_B += s G A^T, grad_A += s B^T G.
//   wan_control_pack  batch -> the patch embedding's GEMM operand [cols | cols] and the flow-match target, one pass, the eager graph's rounding points.
//   wan_patch_lora_*  the launch sequences: fold + ONE NT GEMM (K = Kp, K-extension 2 Kp over the planes) / ONE TN GEMM + the two gradient products.
// The fp32 kernel is not where a step spends time (3 x 2 D r Kp FLOP = 1.8 GF at 1.3B against ~100 TF of block GEMMs): it is written for a fixed
// accumulation order (k ascending, one owner per output, no atomics) and plain 64 x 64 tiles, not tuned.
#include "common.hip.h"
#include "kernels.h"

namespace ftmi {
namespace {

constexpr int kTile = 64, kBK = 16;
constexpr int kLd = kTile + 4;  // floats per k-row of a staged tile: 16-byte aligned rows; the transposing stores of a k-contiguous operand are 2-way conflicted
                                // (k4 * 68 mod 32 takes two values), the ds_read_b128 of the FMA loop are conflict-free (16 lanes = one 256-byte bank row)

struct F32GemmArgs {
    int M, N, K;
    const float* a; long lda_row, lda_col;
    const float* b; long ldb_row, ldb_col;
    float* c; long ldc;
    float scale;
    int accumulate;
    bf16_t* hl; long ld_hl;
    int mode_a, mode_b;  // 0: the reduction index is contiguous (16-byte loads along k), 1: the tile's 64 outer indices are contiguous, 2: neither (scalar loads)
};

// One [kBK][64] tile: element (k, o) lives at src[o * ld_o + k * ld_k].  256 threads x 4 values.
FTMI_DEVICE f32x4 tile_fetch(const float* src, long ld_o, long ld_k, int mode, int tid) {
    if (mode == 0) return *reinterpret_cast<const f32x4*>(src + (long)(tid >> 2) * ld_o + (tid & 3) * 4);
    if (mode == 1) return *reinterpret_cast<const f32x4*>(src + (long)(tid >> 4) * ld_k + (tid & 15) * 4);
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = src[(long)(tid & 63) * ld_o + (long)((tid >> 6) + 4 * i) * ld_k];
    return v;
}
FTMI_DEVICE void tile_put(float* tile, const f32x4& v, int mode, int tid) {
    if (mode == 0) {
        const int o = tid >> 2, k4 = (tid & 3) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[(k4 + i) * kLd + o] = v[i];
    } else if (mode == 1) {
        *reinterpret_cast<f32x4*>(tile + (tid >> 4) * kLd + (tid & 15) * 4) = v;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[((tid >> 6) + 4 * i) * kLd + (tid & 63)] = v[i];
    }
}

// grid (N / 64, M / 64), 256 threads: thread (ty, tx) = (tid / 16, tid % 16) owns the 4 x 4 outputs at rows 4 ty, columns 4 tx of the tile.  The next k-tile
// is fetched into registers while the current one is consumed from LDS.
__global__ __launch_bounds__(256) void f32_gemm_kernel(F32GemmArgs p) {
    __shared__ __attribute__((aligned(16))) float As[kBK * kLd];
    __shared__ __attribute__((aligned(16))) float Bs[kBK * kLd];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * kTile, n0 = blockIdx.x * kTile;
    const float* a0 = p.a + (long)m0 * p.lda_row;
    const float* b0 = p.b + (long)n0 * p.ldb_col;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    f32x4 ra = tile_fetch(a0, p.lda_row, p.lda_col, p.mode_a, tid);
    f32x4 rb = tile_fetch(b0, p.ldb_col, p.ldb_row, p.mode_b, tid);
    for (int k0 = 0; k0 < p.K; k0 += kBK) {
        tile_put(As, ra, p.mode_a, tid);
        tile_put(Bs, rb, p.mode_b, tid);
        __syncthreads();
        if (k0 + kBK < p.K) {
            ra = tile_fetch(a0 + (long)(k0 + kBK) * p.lda_col, p.lda_row, p.lda_col, p.mode_a, tid);
            rb = tile_fetch(b0 + (long)(k0 + kBK) * p.ldb_row, p.ldb_col, p.ldb_row, p.mode_b, tid);
        }
#pragma unroll
        for (int kk = 0; kk < kBK; ++kk) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(As + kk * kLd + ty * 4);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(Bs + kk * kLd + tx * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
    const int n = n0 + tx * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        f32x4* cp = reinterpret_cast<f32x4*>(p.c + (long)m * p.ldc + n);
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p.scale * acc[i][j];
        if (p.accumulate) {
            const f32x4 old = *cp;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = old[j] + v[j];
        }
        *cp = v;
        if (p.hl) {  // the result as two bf16 planes: hi = bf(c), lo = bf(c - hi); hi + lo = c to 2^-18 |c|
            float lo[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) lo[j] = v[j] - rbf(v[j]);
            bf16_t* hp = p.hl + (long)m * p.ld_hl + n;
            *reinterpret_cast<u32x2*>(hp) = u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
            *reinterpret_cast<u32x2*>(hp + p.N) = u32x2{pack2bf(lo[0], lo[1]), pack2bf(lo[2], lo[3])};
        }
    }
}

int operand_mode(const float* ptr, long ld_o, long ld_k) {
    const bool al = (reinterpret_cast<uintptr_t>(ptr) & 15) == 0;
    if (al && ld_k == 1 && ld_o % 4 == 0) return 0;
    if (al && ld_o == 1 && ld_k % 4 == 0) return 1;
    return 2;
}

struct PackArgs {
    ftmi_wan_control_pack_config c;
    const bf16_t *moments, *control, *noise;
    const float *sigmas, *mean, *std;
    const unsigned char* keep;
    bf16_t *cols2, *target;
    long total;  // B C F H W
};

// One thread per latent element (b, c, f, y, x), x fastest: coalesced reads of the mean half of the moments and of the noise, a coalesced target store; the two
// patch-column values (channel c: noisy latent, channel C + c: masked control mean) go out twice each ([cols | cols]) as 2-byte stores, pw of them adjacent.
// 13 x 60 x 104 latents: 1.3 M threads and ~25 MB of traffic per sample batch of 1 -- a few microseconds; it replaces ~10 element-wise / cat / permute passes.
__global__ __launch_bounds__(256) void wan_control_pack_kernel(PackArgs p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total) return;
    const ftmi_wan_control_pack_config& g = p.c;
    const long hw = (long)g.H * g.W;
    long t = idx;
    const int x = (int)(t % g.W); t /= g.W;
    const int y = (int)(t % g.H); t /= g.H;
    const int f = (int)(t % g.F); t /= g.F;
    const int c = (int)(t % g.C);
    const int b = (int)(t / g.C);
    const float mean = p.mean[c], istd = p.std[c];
    const float mu = bf2f(p.moments[(((long)b * 2 * g.C + c) * g.F + f) * hw + (long)y * g.W + x]);
    const float z = rbf((mu - mean) * istd);
    const float nz = bf2f(p.noise[idx]);
    const float sg = p.sigmas[b];
    const bf16_t noisy = f2bf((1.0f - sg) * z + sg * nz);
    p.target[idx] = f2bf(nz - z);
    bf16_t ctrl = 0;
    if (f < g.Fc) {  // a dropped frame is the eager graph's x * 0: a zero with x's sign; frames past the control clip are padding, +0
        ctrl = f2bf((bf2f(p.control[(((long)b * 2 * g.C + c) * g.Fc + f) * hw + (long)y * g.W + x]) - mean) * istd);
        if (!p.keep[(long)b * g.F + f]) ctrl &= 0x8000;
    }
    const int hp = g.H / g.ph, wp = g.W / g.pw, fp = g.F / g.pt;
    const long tok = (long)b * fp * hp * wp + ((long)(f / g.pt) * hp + y / g.ph) * wp + x / g.pw;
    const int sub = ((f % g.pt) * g.ph + y % g.ph) * g.pw + x % g.pw, pv = g.pt * g.ph * g.pw;
    const int kp = 2 * g.C * pv;
    bf16_t* row = p.cols2 + tok * 2 * kp;
    const int c_lat = c * pv + sub, c_ctl = (g.C + c) * pv + sub;
    row[c_lat] = noisy; row[kp + c_lat] = noisy;
    row[c_ctl] = ctrl; row[kp + c_ctl] = ctrl;
}

}  // namespace

int f32_gemm(int M, int N, int K, const float* a, long lda_row, long lda_col, const float* b, long ldb_row, long ldb_col, float* c, long ldc, float scale,
             int accumulate, bf16_t* hl, long ld_hl, hipStream_t st) {
    if (M < 0 || N < 0 || K <= 0) return set_error(FTMI_ERR_INVALID, "f32_gemm: M, N >= 0 and K > 0");
    if (!a || !b || !c) return set_error(FTMI_ERR_INVALID, "f32_gemm: null tensor");
    if (M % 64 || N % 64 || K % 64) return set_error(FTMI_ERR_UNSUPPORTED, "f32_gemm: M, N and K must be multiples of 64");
    if (ldc % 4 || ldc < N || (reinterpret_cast<uintptr_t>(c) & 15)) return set_error(FTMI_ERR_INVALID, "f32_gemm: c needs 16-byte aligned rows of at least N floats");
    if (hl && (ld_hl % 4 || ld_hl < 2L * N || (reinterpret_cast<uintptr_t>(hl) & 7))) return set_error(FTMI_ERR_INVALID, "f32_gemm: the bf16 planes need 8-byte aligned rows of at least 2 N");
    if (M == 0 || N == 0) return 0;
    F32GemmArgs p{M, N, K, a, lda_row, lda_col, b, ldb_row, ldb_col, c, ldc, scale, accumulate, hl, ld_hl, operand_mode(a, lda_row, lda_col), operand_mode(b, ldb_col, ldb_row)};
    hipLaunchKernelGGL(f32_gemm_kernel, dim3(N / 64, M / 64), dim3(256), 0, st, p);
    return check_launch("f32_gemm");
}

int wan_control_pack(const ftmi_wan_control_pack_config& g, const bf16_t* moments, const bf16_t* control, const bf16_t* noise, const float* sigmas, const float* mean,
                     const float* istd, const unsigned char* keep, bf16_t* cols2, bf16_t* target, hipStream_t st) {
    if (g.B <= 0 || g.C <= 0 || g.F <= 0 || g.Fc <= 0 || g.H <= 0 || g.W <= 0 || g.pt <= 0 || g.ph <= 0 || g.pw <= 0)
        return set_error(FTMI_ERR_INVALID, "wan_control_pack: extents must be positive");
    if (g.F % g.pt || g.H % g.ph || g.W % g.pw) return set_error(FTMI_ERR_UNSUPPORTED, "wan_control_pack: the latent size must be whole patches");
    PackArgs p{g, moments, control, noise, sigmas, mean, istd, keep, cols2, target, (long)g.B * g.C * g.F * g.H * g.W};
    if ((p.total + 255) / 256 > 0x7fffffffL) return set_error(FTMI_ERR_UNSUPPORTED, "wan_control_pack: batch too large for one launch");
    hipLaunchKernelGGL(wan_control_pack_kernel, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, st, p);
    return check_launch("wan_control_pack");
}

static int patch_lora_check(const ftmi_wan_patch_lora_config& c, const char* what) {
    if (c.M <= 0 || c.D <= 0 || c.Kp <= 0 || c.r <= 0) return set_error(FTMI_ERR_INVALID, what);
    if (c.r % 64 || c.Kp % 64 || c.D % 64) return set_error(FTMI_ERR_UNSUPPORTED, "wan_patch_lora: r, Kp and D must be multiples of 64");
    return 0;
}

int wan_patch_lora_forward(const ftmi_wan_patch_lora_config& c, const bf16_t* w, const bf16_t* bias, const float* a_f32, const float* b_f32, const bf16_t* cols2,
                           float* dw_f32, bf16_t* w2, bf16_t* out, hipStream_t st) {
    FTMI_TRY(patch_lora_check(c, "wan_patch_lora_forward: bad extent"));
    if (c.refold)  // dW [D, Kp] = s B [D, r] A [r, Kp], and its planes w2 [D, 2 Kp] = [hi | lo]
        FTMI_TRY(f32_gemm(c.D, c.Kp, c.r, b_f32, c.r, 1, a_f32, c.Kp, 1, dw_f32, c.Kp, c.s, 0, w2, 2L * c.Kp, st));
    GemmNtArgs g;  // y = bf(bf(cols W^T + b) + cols hi^T + cols lo^T): the launcher's K-extension rule, x2 = [cols | cols]
    g.X = cols2; g.ldx = 2L * c.Kp; g.W = w; g.ldw = c.Kp; g.M = c.M; g.N = c.D; g.K = c.Kp;
    g.X2 = cols2; g.ldx2 = 2L * c.Kp; g.W2 = w2; g.ldw2 = 2L * c.Kp; g.K2 = 2 * c.Kp;
    g.bias = bias; g.out = out; g.ldo = c.D; g.epi = EPI_STORE; g.variant = c.gemm_variant;
    return gemm_nt(g, st);
}

int wan_patch_lora_backward(const ftmi_wan_patch_lora_config& c, const float* a_f32, const float* b_f32, const bf16_t* cols2, const bf16_t* dx0, float* g_ws,
                            float* grad_a, float* grad_b, hipStream_t st) {
    FTMI_TRY(patch_lora_check(c, "wan_patch_lora_backward: bad extent"));
    if (hipMemsetAsync(g_ws, 0, sizeof(float) * (size_t)c.D * c.Kp, st) != hipSuccess) return set_error(FTMI_ERR_LAUNCH, "wan_patch_lora_backward: memset failed");
    GemmTnArgs t;  // G [D, Kp] = dx0^T cols
    t.U = dx0; t.ldu = c.D; t.V = cols2; t.ldv = 2L * c.Kp; t.C = g_ws; t.ldc = c.Kp; t.M = c.M; t.P = c.D; t.Q = c.Kp;
    FTMI_TRY(gemm_tn(t, st));
    // grad_B [D, r] += s G A^T (b(k, n) = A[n, k]);  grad_A [r, Kp] += s B^T G (a(m, k) = B[k, m])
    FTMI_TRY(f32_gemm(c.D, c.r, c.Kp, g_ws, c.Kp, 1, a_f32, 1, c.Kp, grad_b, c.r, c.s, 1, nullptr, 0, st));
    return f32_gemm(c.r, c.Kp, c.D, b_f32, 1, c.r, g_ws, c.Kp, 1, grad_a, c.Kp, c.s, 1, nullptr, 0, st);
}

}  // namespace ftmi
