// HBM-bound kernels of the LTX-Video LoRA SFT step (gfx950): normalisation + AdaLN modulation,
// QK-RMSNorm + RoPE, gate multiply, noising/patchify, loss, timestep embedding, and their backward.
// Every kernel rounds through bf16 exactly where the reference's eager bf16 graph materialises a
// tensor (each torch op = fp32 internal math, one rounding at its output), so fusing the chain into
// one pass over HBM does not move rounding points.  All loads/stores are 16-byte vectors; one
// 64-lane wavefront owns one token row and reduces with cross-lane shuffles (no LDS).
//
// Replaces (reference call sites): RMSNorm/LayerNorm + scale/shift of LTXVideoTransformerBlock and the
// tail of patches/models/ltx_video/patch.py:118-123; patches/dependencies/diffusers/rms_norm.py:17-29;
// apply_rotary_emb patch.py:23-33; models/ltx_video/base_specification.py:295-320,427-459;
// functional/diffusion.py:4-11; trainer/sft_trainer/trainer.py:463-481 (loss).
#include <utility>

#include "common.hip.h"
#include "kernels.h"

namespace ftmi {

static constexpr int kNch = 4;  // 16-byte chunks per lane: row width 64 * 8 * 4 = 2048

FTMI_DEVICE void unpack8(const s16x8& v, float (&f)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = bf2f((bf16_t)v[e]);
}
FTMI_DEVICE s16x8 pack8(const float (&f)[8]) {
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = pack2bf(f[2 * e], f[2 * e + 1]);
    return __builtin_bit_cast(s16x8, w);
}

// ---------------------------------------------------------------------------------------------------
__global__ void ada_prep_kernel(const bf16_t* __restrict__ tables, const bf16_t* __restrict__ temb, bf16_t* __restrict__ ada,
                                int L, int B, int D) {
    const long n = (long)L * B * D;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
        const int d = (int)(idx % D);
        const int b = (int)((idx / D) % B);
        const int l = (int)(idx / ((long)D * B));
        bf16_t* o = ada + ((long)(l * B + b) * 8) * D + d;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            float v = rbf(bf2f(tables[((long)l * 6 + i) * D + d]) + bf2f(temb[(long)b * 6 * D + (long)i * D + d]));
            o[(long)i * D] = f2bf(v);
            if (i == 1) o[(long)6 * D] = f2bf(1.0f + v);
            if (i == 4) o[(long)7 * D] = f2bf(1.0f + v);
        }
    }
}
int ada_prep(const bf16_t* tables, const bf16_t* temb, bf16_t* ada, int L, int B, int D, hipStream_t st) {
    const long n = (long)L * B * D;
    if (L <= 0 || B <= 0 || D <= 0) return 0;
    hipLaunchKernelGGL(ada_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tables, temb, ada, L, B, D);
    return check_launch("ada_prep");
}

__global__ void ada_out_prep_kernel(const bf16_t* __restrict__ table2, const bf16_t* __restrict__ emb, bf16_t* __restrict__ out, int B, int D) {
    const long n = (long)B * D;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
        const int d = (int)(idx % D), b = (int)(idx / D);
        const float e = bf2f(emb[(long)b * D + d]);
        const float shift = rbf(bf2f(table2[d]) + e);
        const float scale = rbf(bf2f(table2[D + d]) + e);
        bf16_t* o = out + (long)b * 3 * D + d;
        o[0] = f2bf(shift);
        o[D] = f2bf(scale);
        o[2 * D] = f2bf(1.0f + scale);
    }
}
int ada_out_prep(const bf16_t* table2, const bf16_t* emb, bf16_t* ada_out, int B, int D, hipStream_t st) {
    const long n = (long)B * D;
    if (B <= 0 || D <= 0) return 0;
    hipLaunchKernelGGL(ada_out_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, table2, emb, ada_out, B, D);
    return check_launch("ada_out_prep");
}

// ---------------------------------------------------------------------------------------------------
// Valid width of a zero-padded row (round 6: the reference's DUMMY model -- 4 heads x 8, tests/models/ltx_video/base_specification.py:47-58 -- runs through these
// kernels embedded in the 2048-wide layout: every weight zero-padded, so every padded channel carries exact zeros; what a normalisation must still know is how many
// channels the mean is taken over).  Set by the DiT pass around its launches (one process per GPU, one pass at a time per thread); 0 = the whole row.
static thread_local int g_valid_width = 0;
void rowwise_set_valid_width(int dv) { g_valid_width = dv; }
static inline int valid_width(int D) { return g_valid_width > 0 && g_valid_width < D ? g_valid_width : D; }

template <bool LN>
__global__ __launch_bounds__(256) void norm_modulate_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ shift,
                                                                const bf16_t* __restrict__ onep, long mod_bstride,
                                                                bf16_t* __restrict__ y, int rows, int rows_per_batch, float eps, int Dv) {
    constexpr int D = kNch * 512;
    const float invD = 1.0f / Dv;  // (Dv = D unless the row is a zero-padded narrow one)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = row / rows_per_batch;
    const bf16_t* xp = x + (long)row * D;
    float xv[kNch][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int it = 0; it < kNch; ++it) {
        s16x8 raw = *reinterpret_cast<const s16x8*>(xp + (lane + 64 * it) * 8);
        unpack8(raw, xv[it]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            s1 += xv[it][e];
            s2 += xv[it][e] * xv[it][e];
        }
    }
    float mean = 0.f, rstd;
    if (LN) {
        mean = wave_sum(s1) * invD;
        float v = 0.f;
#pragma unroll
        for (int it = 0; it < kNch; ++it)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float c = xv[it][e] - mean;
                if ((lane + 64 * it) * 8 + e < Dv) v += c * c;  // the padded zeros are not part of the row (taking their mean^2 out of the full sum afterwards cancels)
            }
        rstd = rsqrtf(wave_sum(v) * invD + eps);
    } else {
        rstd = rsqrtf(wave_sum(s2) * invD + eps);
    }
    const bf16_t* sp = shift + (long)b * mod_bstride;
    const bf16_t* op = onep + (long)b * mod_bstride;
    bf16_t* yp = y + (long)row * D;
#pragma unroll
    for (int it = 0; it < kNch; ++it) {
        const int off = (lane + 64 * it) * 8;
        float sv[8], ov[8], o[8];
        unpack8(*reinterpret_cast<const s16x8*>(sp + off), sv);
        unpack8(*reinterpret_cast<const s16x8*>(op + off), ov);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float n = rbf((xv[it][e] - mean) * rstd);
            o[e] = rbf(n * ov[e]) + sv[e];
            if (LN && off + e >= Dv) o[e] = 0.f;
        }
        *reinterpret_cast<s16x8*>(yp + off) = pack8(o);
    }
}
int norm_modulate_fwd(const bf16_t* x, const bf16_t* shift, const bf16_t* onep, long mod_bstride, bf16_t* y, int rows,
                      int rows_per_batch, int D, float eps, int layernorm, hipStream_t st) {
    if (D != kNch * 512) return set_error(FTMI_ERR_UNSUPPORTED, "norm_modulate: row width must be 2048");
    if (rows <= 0) return 0;  // (an empty range: nothing to launch, like the Wan and CogVideoX launchers)
    dim3 grid((rows + 3) / 4);
    if (layernorm)
        hipLaunchKernelGGL(norm_modulate_fwd_kernel<true>, grid, dim3(256), 0, st, x, shift, onep, mod_bstride, y, rows, rows_per_batch, eps, valid_width(D));
    else
        hipLaunchKernelGGL(norm_modulate_fwd_kernel<false>, grid, dim3(256), 0, st, x, shift, onep, mod_bstride, y, rows, rows_per_batch, eps, valid_width(D));
    return check_launch("norm_modulate_fwd");
}

template <bool LN>
__global__ __launch_bounds__(256) void norm_modulate_bwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                                const bf16_t* __restrict__ onep, long mod_bstride,
                                                                const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx, int rows,
                                                                int rows_per_batch, float eps, const bf16_t* __restrict__ gate2, long gate2_bstride,
                                                                bf16_t* __restrict__ dx2, int Dv) {
    constexpr int D = kNch * 512;
    const float invD = 1.0f / Dv;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = row / rows_per_batch;
    const bf16_t* xp = x + (long)row * D;
    const bf16_t* dyp = dy + (long)row * D;
    const bf16_t* op = onep + (long)b * mod_bstride;
    float xv[kNch][8], gv[kNch][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int it = 0; it < kNch; ++it) {
        const int off = (lane + 64 * it) * 8;
        unpack8(*reinterpret_cast<const s16x8*>(xp + off), xv[it]);
        float dv[8], ov[8];
        unpack8(*reinterpret_cast<const s16x8*>(dyp + off), dv);
        unpack8(*reinterpret_cast<const s16x8*>(op + off), ov);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            gv[it][e] = rbf(dv[e] * ov[e]);  // grad w.r.t. the normalised tensor (a bf16 tensor in the eager graph)
            s1 += xv[it][e];
            s2 += xv[it][e] * xv[it][e];
        }
    }
    float mean = 0.f, rstd;
    if (LN) {
        mean = wave_sum(s1) * invD;
        float v = 0.f;
#pragma unroll
        for (int it = 0; it < kNch; ++it)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float c = xv[it][e] - mean;
                if ((lane + 64 * it) * 8 + e < Dv) v += c * c;
            }
        rstd = rsqrtf(wave_sum(v) * invD + eps);
    } else {
        rstd = rsqrtf(wave_sum(s2) * invD + eps);
    }
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int it = 0; it < kNch; ++it)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float xh = (xv[it][e] - mean) * rstd;
            c1 += gv[it][e];
            c2 += gv[it][e] * xh;
        }
    // (padded channels: their upstream gradient is an exact zero -- zero weight columns -- so they add nothing to c1 / c2; what LayerNorm's mean would hand back to them
    //  is masked below: a padded channel does not exist)
    c1 = LN ? wave_sum(c1) * invD : 0.f;
    c2 = wave_sum(c2) * invD;
    bf16_t* dxp = dx + (long)row * D;
#pragma unroll
    for (int it = 0; it < kNch; ++it) {
        const int off = (lane + 64 * it) * 8;
        float rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, o[8];
        if (dres) unpack8(*reinterpret_cast<const s16x8*>(dres + (long)row * D + off), rv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float xh = (xv[it][e] - mean) * rstd;
            float d = rstd * (gv[it][e] - c1 - xh * c2);
            o[e] = dres ? rv[e] + rbf(d) : d;
            if (LN && off + e >= Dv) o[e] = 0.f;
        }
        *reinterpret_cast<s16x8*>(dxp + off) = pack8(o);
        if (dx2) {  // the consumer's first op, bf(dx * gate[b]) (a gate multiply), done here while dx is in registers: one pass and one launch less
            float g2[8], o2[8];
            unpack8(*reinterpret_cast<const s16x8*>(gate2 + (long)b * gate2_bstride + off), g2);
#pragma unroll
            for (int e = 0; e < 8; ++e) o2[e] = rbf(o[e]) * g2[e];
            *reinterpret_cast<s16x8*>(dx2 + (long)row * D + off) = pack8(o2);
        }
    }
}
int norm_modulate_bwd(const bf16_t* x, const bf16_t* dy, const bf16_t* onep, long mod_bstride, const bf16_t* dres, bf16_t* dx,
                      int rows, int rows_per_batch, int D, float eps, int layernorm, hipStream_t st, const bf16_t* gate2, long gate2_bstride,
                      bf16_t* dx2) {
    if (D != kNch * 512) return set_error(FTMI_ERR_UNSUPPORTED, "norm_modulate: row width must be 2048");
    if (rows <= 0) return 0;  // (an empty range: nothing to launch, like the Wan and CogVideoX launchers)
    dim3 grid((rows + 3) / 4);
    if (layernorm)
        hipLaunchKernelGGL(norm_modulate_bwd_kernel<true>, grid, dim3(256), 0, st, x, dy, onep, mod_bstride, dres, dx, rows, rows_per_batch, eps, gate2, gate2_bstride, dx2, valid_width(D));
    else
        hipLaunchKernelGGL(norm_modulate_bwd_kernel<false>, grid, dim3(256), 0, st, x, dy, onep, mod_bstride, dres, dx, rows, rows_per_batch, eps, gate2, gate2_bstride, dx2, valid_width(D));
    return check_launch("norm_modulate_bwd");
}

// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qknorm_rope_fwd_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ w,
                                                              const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                              bf16_t* __restrict__ y, long ldy, int rows, int rows_per_batch, float eps, int w_rows,
                                                              const bf16_t* __restrict__ x2, const bf16_t* __restrict__ w2, bf16_t* __restrict__ y2, int Dv) {
    constexpr int D = kNch * 512;
    if (blockIdx.y == 1) {  // pair launch (q and k of one projection): same strides and RoPE rows, second tensor set
        x = x2; w = w2; y = y2;
    }
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int s = row % rows_per_batch;
    if (w_rows > 1) w += (long)(row % w_rows) * D;
    const bf16_t* xp = x + (long)row * ldx;
    float xv[kNch][8];
    float s2 = 0.f;
#pragma unroll
    for (int it = 0; it < kNch; ++it) {
        unpack8(*reinterpret_cast<const s16x8*>(xp + (lane + 64 * it) * 8), xv[it]);
#pragma unroll
        for (int e = 0; e < 8; ++e) s2 += xv[it][e] * xv[it][e];
    }
    const float rstd = rsqrtf(wave_sum(s2) * (1.0f / Dv) + eps);
    bf16_t* yp = y + (long)row * ldy;
#pragma unroll
    for (int it = 0; it < kNch; ++it) {
        const int ch = lane + 64 * it;
        float wv[8], n[8], o[8];
        unpack8(*reinterpret_cast<const s16x8*>(w + ch * 8), wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) n[e] = rbf(xv[it][e] * rstd * wv[e]);
        if (cos_t) {
            f32x4 c = *reinterpret_cast<const f32x4*>(cos_t + (long)s * (D / 2) + ch * 4);
            f32x4 sn = *reinterpret_cast<const f32x4*>(sin_t + (long)s * (D / 2) + ch * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[2 * k] = n[2 * k] * c[k] + (-n[2 * k + 1]) * sn[k];
                o[2 * k + 1] = n[2 * k + 1] * c[k] + n[2 * k] * sn[k];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = n[e];
        }
        *reinterpret_cast<s16x8*>(yp + ch * 8) = pack8(o);
    }
}
int qknorm_rope_fwd(const bf16_t* x, long ldx, const bf16_t* w, const float* cos_t, const float* sin_t, bf16_t* y, long ldy,
                    int rows, int rows_per_batch, int D, float eps, hipStream_t st, int w_rows, const bf16_t* x2, const bf16_t* w2, bf16_t* y2) {
    if (D != kNch * 512) return set_error(FTMI_ERR_UNSUPPORTED, "qknorm_rope: row width must be 2048");
    if ((ldx % 8) || (ldy % 8)) return set_error(FTMI_ERR_INVALID, "qknorm_rope: row strides must keep 16-byte alignment");
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(qknorm_rope_fwd_kernel, dim3((rows + 3) / 4, x2 ? 2 : 1), dim3(256), 0, st, x, ldx, w, cos_t, sin_t, y, ldy, rows, rows_per_batch, eps, w_rows,
                       x2, w2, y2, valid_width(D));
    return check_launch("qknorm_rope_fwd");
}

__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ w,
                                                              const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                              const bf16_t* __restrict__ dy, long lddy, bf16_t* __restrict__ dx, long lddx,
                                                              int rows, int rows_per_batch, float eps, int w_rows, const bf16_t* __restrict__ x2,
                                                              const bf16_t* __restrict__ w2, const bf16_t* __restrict__ dy2, bf16_t* __restrict__ dx2,
                                                              int row_grp, int row_grp_span, int Dv) {
    constexpr int D = kNch * 512;
    if (blockIdx.y == 1) {
        x = x2; w = w2; dy = dy2; dx = dx2;
    }
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int s = row % rows_per_batch;
    if (w_rows > 1) w += (long)(row % w_rows) * D;
    // rows may live in groups: row i sits at position (i / row_grp) * row_grp_span + i % row_grp (a block range of the (token, block) arrays)
    const long mrow = row_grp > 0 ? (long)(row / row_grp) * row_grp_span + row % row_grp : (long)row;
    const bf16_t* xp = x + mrow * ldx;
    const bf16_t* dyp = dy + mrow * lddy;
    float xv[kNch][8], gv[kNch][8];
    float s2 = 0.f;
#pragma unroll
    for (int it = 0; it < kNch; ++it) {
        const int ch = lane + 64 * it;
        unpack8(*reinterpret_cast<const s16x8*>(xp + ch * 8), xv[it]);
        float dv[8], wv[8], dn[8];
        unpack8(*reinterpret_cast<const s16x8*>(dyp + ch * 8), dv);
        unpack8(*reinterpret_cast<const s16x8*>(w + ch * 8), wv);
        if (cos_t) {
            f32x4 c = *reinterpret_cast<const f32x4*>(cos_t + (long)s * (D / 2) + ch * 4);
            f32x4 sn = *reinterpret_cast<const f32x4*>(sin_t + (long)s * (D / 2) + ch * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // autograd of (x.float()*cos + rot(x).float()*sin).to(bf16): each branch's grad is cast to bf16
                // before the two are accumulated (in bf16) into x's grad
                dn[2 * k] = rbf(rbf(dv[2 * k] * c[k]) + rbf(dv[2 * k + 1] * sn[k]));
                dn[2 * k + 1] = rbf(rbf(dv[2 * k + 1] * c[k]) + (-rbf(dv[2 * k] * sn[k])));
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) dn[e] = dv[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            gv[it][e] = dn[e] * wv[e];
            s2 += xv[it][e] * xv[it][e];
        }
    }
    const float rstd = rsqrtf(wave_sum(s2) * (1.0f / Dv) + eps);
    float c2 = 0.f;
#pragma unroll
    for (int it = 0; it < kNch; ++it)
#pragma unroll
        for (int e = 0; e < 8; ++e) c2 += gv[it][e] * (xv[it][e] * rstd);
    c2 = wave_sum(c2) * (1.0f / Dv);
    bf16_t* dxp = dx + mrow * lddx;
#pragma unroll
    for (int it = 0; it < kNch; ++it) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = rstd * (gv[it][e] - (xv[it][e] * rstd) * c2);
        *reinterpret_cast<s16x8*>(dxp + (lane + 64 * it) * 8) = pack8(o);
    }
}
int qknorm_rope_bwd(const bf16_t* x, long ldx, const bf16_t* w, const float* cos_t, const float* sin_t, const bf16_t* dy, long lddy,
                    bf16_t* dx, long lddx, int rows, int rows_per_batch, int D, float eps, hipStream_t st, int w_rows, const bf16_t* x2, const bf16_t* w2,
                    const bf16_t* dy2, bf16_t* dx2, int row_grp, int row_grp_span) {
    if (D != kNch * 512) return set_error(FTMI_ERR_UNSUPPORTED, "qknorm_rope: row width must be 2048");
    if ((ldx % 8) || (lddy % 8) || (lddx % 8)) return set_error(FTMI_ERR_INVALID, "qknorm_rope: row strides must keep 16-byte alignment");
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(qknorm_rope_bwd_kernel, dim3((rows + 3) / 4, x2 ? 2 : 1), dim3(256), 0, st, x, ldx, w, cos_t, sin_t, dy, lddy, dx, lddx, rows, rows_per_batch, eps, w_rows,
                       x2, w2, dy2, dx2, row_grp, row_grp_span, valid_width(D));
    return check_launch("qknorm_rope_bwd");
}

// ---------------------------------------------------------------------------------------------------
// latents [B][C][S] -> (x_t, target) [B][S][C]:  normalise, flow-match mix, patchify (p = p_t = 1)
__global__ __launch_bounds__(256) void noise_pack_kernel(const bf16_t* __restrict__ lat, const bf16_t* __restrict__ noise,
                                                         const float* __restrict__ mean, const float* __restrict__ std_,
                                                         const float* __restrict__ sigma, const float* __restrict__ sigma_first,
                                                         int first_frame_tokens, bf16_t* __restrict__ xt, bf16_t* __restrict__ target,
                                                         int C, int S) {
    // tile: 64 channels x 64 tokens, LDS pitch 66 (2-byte elements) to spread the column reads
    __shared__ bf16_t txt[64][66];
    __shared__ bf16_t ttg[64][66];
    const int b = blockIdx.z, c0 = blockIdx.y * 64, s0 = blockIdx.x * 64;
    const float sg = sigma[b];
    const float sgf = sigma_first ? sigma_first[b] : sg;
    for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
        const int cl = idx >> 6, sl = idx & 63;
        const int c = c0 + cl, s = s0 + sl;
        bf16_t vx = 0, vt = 0;
        if (c < C && s < S) {
            const long off = ((long)b * C + c) * S + s;
            const float x0 = rbf((bf2f(lat[off]) - mean[c]) * 1.0f / std_[c]);
            const float n = bf2f(noise[off]);
            const float t = (s < first_frame_tokens) ? sgf : sg;
            vx = f2bf((1.0f - t) * x0 + t * n);
            vt = f2bf(n - x0);
        }
        txt[cl][sl] = vx;
        ttg[cl][sl] = vt;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
        const int sl = idx >> 6, cl = idx & 63;
        const int c = c0 + cl, s = s0 + sl;
        if (c < C && s < S) {
            const long off = ((long)b * S + s) * C + c;
            xt[off] = txt[cl][sl];
            target[off] = ttg[cl][sl];
        }
    }
}
int noise_pack(const bf16_t* latents, const bf16_t* noise, const float* mean, const float* std_, const float* sigma,
               const float* sigma_first, int first_frame_tokens, bf16_t* xt, bf16_t* target, int B, int C, int S, hipStream_t st) {
    if (B <= 0 || C <= 0 || S <= 0) return 0;  // nothing to write: no launch (an empty grid is a launch error)
    dim3 grid((S + 63) / 64, (C + 63) / 64, B);
    hipLaunchKernelGGL(noise_pack_kernel, grid, dim3(256), 0, st, latents, noise, mean, std_, sigma, sigma_first, first_frame_tokens, xt,
                       target, C, S);
    return check_launch("noise_pack");
}

// ---------------------------------------------------------------------------------------------------
// loss = mean_b mean_{s,c} w_b (pred - target)^2 ; dpred = bf(2 w_b (pred - target) / (per_sample * B))
__global__ __launch_bounds__(256) void mse_loss_kernel(const bf16_t* __restrict__ pred, const bf16_t* __restrict__ target,
                                                       const float* __restrict__ weight, float* __restrict__ loss, bf16_t* __restrict__ dpred,
                                                       long per_sample, float inv_count, float grad_scale) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const float w = weight ? weight[b] : 1.0f;
    const long nch = per_sample / 8;
    float acc = 0.f;
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < nch; c += (long)gridDim.x * blockDim.x) {
        const long off = (long)b * per_sample + c * 8;
        float pv[8], tv[8], o[8];
        unpack8(*reinterpret_cast<const s16x8*>(pred + off), pv);
        unpack8(*reinterpret_cast<const s16x8*>(target + off), tv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = pv[e] - tv[e];
            acc += w * (d * d);
            o[e] = (w * (2.0f * d)) * grad_scale;
        }
        if (dpred) *reinterpret_cast<s16x8*>(dpred + off) = pack8(o);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    // one partial per workgroup, summed in a FIXED order by mse_loss_finish_kernel: the logged loss is bitwise reproducible (an atomicAdd here made
    // two ranks that computed the same step report losses one ulp apart)
    if (threadIdx.x == 0) loss[blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1] + red[2] + red[3]) * inv_count;
}
__global__ __launch_bounds__(64) void mse_loss_finish_kernel(const float* __restrict__ partials, int n, float* __restrict__ loss) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) acc += partials[i];  // lane l: partials l, l + 64, ... in order
    acc = wave_sum(acc);                                            // fixed butterfly
    if (threadIdx.x == 0) *loss = acc;
}
int mse_loss_fwd_bwd(const bf16_t* pred, const bf16_t* target, const float* weight, float* loss, bf16_t* dpred, int B, long per_sample,
                     float grad_scale, float* partials, hipStream_t st) {
    if (B <= 0 || per_sample <= 0) return set_error(FTMI_ERR_INVALID, "mse_loss: the mean over no element is not defined");
    if (per_sample % 8) return set_error(FTMI_ERR_UNSUPPORTED, "mse_loss: per-sample size % 8");
    long blocks = (per_sample / 8 + 255) / 256;
    if (blocks > FTMI_MSE_SCRATCH_FLOATS_PER_SAMPLE) blocks = FTMI_MSE_SCRATCH_FLOATS_PER_SAMPLE;
    // per-workgroup partials live in CALLER-owned scratch (>= FTMI_MSE_SCRATCH_FLOATS_PER_SAMPLE * B floats): nothing is allocated on the launch
    // path, so the call is legal during stream capture and never synchronises the device
    const long need = blocks * B;
    const float inv_count = 1.0f / ((float)per_sample * (float)B);
    hipLaunchKernelGGL(mse_loss_kernel, dim3((unsigned)blocks, B), dim3(256), 0, st, pred, target, weight, partials, dpred, per_sample, inv_count,
                       inv_count * grad_scale);
    hipLaunchKernelGGL(mse_loss_finish_kernel, dim3(1), dim3(64), 0, st, partials, (int)need, loss);
    return check_launch("mse_loss");
}

// ---------------------------------------------------------------------------------------------------
__global__ void timestep_sinusoid_kernel(const float* __restrict__ tval, bf16_t* __restrict__ out, int B) {
    const int b = blockIdx.x, k = threadIdx.x;  // 256 threads: [cos(128) | sin(128)]
    if (b >= B) return;
    const float t = tval[b];
    const int j = k & 127;
    const float freq = expf(-9.210340371976184f * (float)j / 128.0f);
    const float a = t * freq;
    out[(long)b * 256 + k] = f2bf(k < 128 ? cosf(a) : sinf(a));
}
int timestep_sinusoid(const float* tval, bf16_t* out, int B, hipStream_t st) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(timestep_sinusoid_kernel, dim3(B), dim3(256), 0, st, tval, out, B);
    return check_launch("timestep_sinusoid");
}

// y[r][n] = bf(sum_k xin[r][k] W[n][k] + bias[n]),  xin = silu_in ? bf(silu(x)) : x ;  rows <= 8, one wave per n
template <int R>
__global__ __launch_bounds__(256) void small_linear_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W,
                                                           const bf16_t* __restrict__ bias, bf16_t* __restrict__ y, int N, int K, int silu_in) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        float wv[8];
        unpack8(*reinterpret_cast<const s16x8*>(W + (long)n * K + k), wv);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float xv[8];
            unpack8(*reinterpret_cast<const s16x8*>(x + (long)r * K + k), xv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float xin = silu_in ? rbf(silu_f(xv[e])) : xv[e];
                acc[r] += xin * wv[e];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float s = wave_sum(acc[r]);
        if (lane == 0) y[(long)r * N + n] = f2bf(s + (bias ? bf2f(bias[n]) : 0.f));
    }
}
int small_linear(const bf16_t* x, const bf16_t* W, const bf16_t* bias, bf16_t* y, int rows, int N, int K, int silu_in, int silu_out,
                 hipStream_t st) {
    (void)silu_out;
    if (K % 8) return set_error(FTMI_ERR_UNSUPPORTED, "small_linear: K % 8");
    if (rows < 1 || rows > 8) return set_error(FTMI_ERR_UNSUPPORTED, "small_linear: rows must be 1..8");
    if (N <= 0) return 0;
    dim3 grid((N + 3) / 4);
#define FTMI_SL(R)                                                                                             \
    case R:                                                                                                    \
        hipLaunchKernelGGL(small_linear_kernel<R>, grid, dim3(256), 0, st, x, W, bias, y, N, K, silu_in);      \
        break;
    switch (rows) {
        FTMI_SL(1) FTMI_SL(2) FTMI_SL(3) FTMI_SL(4) FTMI_SL(5) FTMI_SL(6) FTMI_SL(7) FTMI_SL(8)
        default:
            return set_error(FTMI_ERR_UNSUPPORTED, "small_linear: rows must be 1..8");
    }
#undef FTMI_SL
    return check_launch("small_linear");
}

// ---------------------------------------------------------------------------------------------------
// optimiser: global grad-norm clip + AdamW over the flat LoRA buffer (reference: utils/torch.py:99-161 clip,
// torch.optim.AdamW(fused=False) via optimizer.py:117-125)
// Deterministic: every block leaves its partial sum in scratch[2 + block]; the block that takes the last ticket adds the partials in a
// fixed order.  (A float atomicAdd per block gave totals that differed in the last bit from run to run -- and therefore between the
// ranks of a data-parallel job, whose clip coefficients and parameters would then drift apart.)
static constexpr int kSumsqMaxBlocks = 2048;  // = FTMI_CLIP_SCRATCH_FLOATS - 2
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long n, float* __restrict__ out) {
    __shared__ float red[4];
    __shared__ bool last;
    float acc = 0.f;
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 v = *reinterpret_cast<const f32x4*>(g + i * 4);
        acc += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long i = n4 * 4; i < n; ++i) acc += g[i] * g[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        out[2 + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        __threadfence();
        last = atomicAdd(reinterpret_cast<unsigned*>(out) + 1, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    float t = 0.f;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) t += __hip_atomic_load(out + 2 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // device-scope load, fixed order per thread
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}
int sumsq(const float* g, long n, float* out, hipStream_t st) {
    long blocks = (n / 4 + 255) / 256;
    if (blocks > kSumsqMaxBlocks) blocks = kSumsqMaxBlocks;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g, n, out);
    return check_launch("sumsq");
}

// In-place global-norm clip (utils/torch.py:99-161 as trainer.py:487-492 calls it after EVERY backward, also on the micro-steps of a
// gradient-accumulation window, where the optimiser does not step): g *= min(1, max_norm / (norm + 1e-6)).  Nothing is touched when the
// norm is inside the bound (the usual case): every block reads the scalar and leaves.
__global__ __launch_bounds__(256) void clip_scale_kernel(float* __restrict__ g, long n, const float* __restrict__ sumsq_in, float max_norm,
                                                         float* __restrict__ grad_norm_out) {
    const float total_norm = sqrtf(*sumsq_in);
    if (grad_norm_out && blockIdx.x == 0 && threadIdx.x == 0) *grad_norm_out = total_norm;
    const float coef = max_norm / (total_norm + 1e-6f);
    if (!(coef < 1.0f) || max_norm <= 0.f) return;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) g[i] *= coef;
}
int clip_scale(float* g, long n, const float* sumsq_in, float max_norm, float* grad_norm_out, hipStream_t st) {
    if (n <= 0) return 0;
    long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(clip_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g, n, sumsq_in, max_norm, grad_norm_out);
    return check_launch("clip_scale");
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, const float* __restrict__ sumsq_in, float max_norm,
                                                    float lr, float beta1, float beta2, float eps, float wd, float bc1, float bc2_sqrt,
                                                    float* __restrict__ grad_norm_out) {
    const float total_norm = sqrtf(*sumsq_in);
    float coef = max_norm / (total_norm + 1e-6f);
    coef = coef > 1.0f ? 1.0f : coef;
    if (max_norm <= 0.f) coef = 1.0f;
    if (grad_norm_out && blockIdx.x == 0 && threadIdx.x == 0) *grad_norm_out = total_norm;
    const float step_size = lr / bc1;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float gi = g[i] * coef;
        float pi = p[i] * (1.0f - lr * wd);
        const float mi = m[i] + (gi - m[i]) * (1.0f - beta1);  // exp_avg.lerp_(grad, 1 - beta1)
        const float vi = v[i] * beta2 + (1.0f - beta2) * gi * gi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        pi = pi - step_size * (mi / denom);
        p[i] = pi;
        m[i] = mi;
        v[i] = vi;
    }
}
int adamw_clip_step(float* p, const float* g, float* m, float* v, long n, const float* sumsq_in, float max_norm, float lr, float beta1,
                    float beta2, float eps, float wd, int step, float* grad_norm_out, hipStream_t st) {
    if (n <= 0) return 0;
    // bias corrections in double from the fp32 betas, like adamw_bf16_step: powf alone is off by up to 7e-6 relative in 1 - beta2^step at small steps
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p, g, m, v, n, sumsq_in, max_norm, lr, beta1, beta2, eps, wd,
                       bc1, bc2_sqrt, grad_norm_out);
    return check_launch("adamw");
}

// AdamW on bf16 parameters with bf16 moments: what torch.optim.AdamW does to a model that is trained in bf16 (the reference's full fine-tune,
// BASELINE config 4: transformer_dtype bf16, optimizer.py:17-46) -- every torch op of the update is one fp32 computation rounded to bf16:
//   p *= 1 - lr wd;  m = lerp(m, g, 1 - b1);  v *= b2;  v += (1 - b2) g g;  d = sqrt(v);  d /= sqrt(bc2);  d += eps;  p += -(lr / bc1) m / d
// g arrives in fp32 (the reduce-scattered gradient shard) and is scaled by the clip coefficient and rounded to bf16 first: the reference's
// sharded gradient is a bf16 tensor (FSDP-2 casts the fp32 reduce result back to the parameter dtype) that clip_grad_norm_ multiplies in place.
__global__ __launch_bounds__(256) void adamw_bf16_kernel(bf16_t* __restrict__ p, const float* __restrict__ g, bf16_t* __restrict__ m,
                                                         bf16_t* __restrict__ v, long n, const float* __restrict__ sumsq_in, float max_norm, float decay,
                                                         float w1, float beta2, float omb2, float eps, float step_size, float bc2_sqrt,
                                                         float* __restrict__ grad_norm_out) {
    float coef = 1.0f;
    if (sumsq_in) {
        const float total_norm = sqrtf(*sumsq_in);
        coef = fminf(max_norm / (total_norm + 1e-6f), 1.0f);
        if (max_norm <= 0.f) coef = 1.0f;  // no clip, as in adamw_kernel and clip_scale
        if (grad_norm_out && blockIdx.x == 0 && threadIdx.x == 0) *grad_norm_out = total_norm;
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float gi = rbf(g[i]);
        if (coef < 1.0f) gi = rbf(gi * coef);
        float pi = rbf(bf2f(p[i]) * decay);
        const float mi0 = bf2f(m[i]);
        const float mi = rbf(w1 < 0.5f ? mi0 + w1 * (gi - mi0) : gi - (gi - mi0) * (1.0f - w1));  // at::lerp
        float vi = rbf(bf2f(v[i]) * beta2);
        vi = rbf(vi + omb2 * gi * gi);
        float d = rbf(sqrtf(vi));
        d = rbf(d / bc2_sqrt);
        d = rbf(d + eps);
        pi = rbf(pi + step_size * (mi / d));
        p[i] = f2bf(pi);
        m[i] = f2bf(mi);
        v[i] = f2bf(vi);
    }
}
int adamw_bf16_step(bf16_t* p, const float* g, bf16_t* m, bf16_t* v, long n, const float* sumsq_in, float max_norm, float lr, float beta1,
                    float beta2, float eps, float wd, int step, float* grad_norm_out, hipStream_t st) {
    if (n <= 0) return 0;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(adamw_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p, g, m, v, n, sumsq_in, max_norm, (float)(1.0 - (double)lr * wd),
                       (float)(1.0 - (double)beta1), beta2, (float)(1.0 - (double)beta2), eps, (float)(-((double)lr / bc1)), (float)sqrt(bc2), grad_norm_out);
    return check_launch("adamw_bf16");
}

// ---------------------------------------------------------------------------------------------------
// CogVideoX spec-level elementwise ops: DDIM add_noise / get_velocity as CogVideoXModelSpecification.forward applies them
// (finetrainers/models/cogvideox/base_specification.py:283-293,326-329 around [upstream] CogVideoXDDIMScheduler).  One kernel does both
// forms (mode 0: x0 = bf(lat * scale); out = bf(bf(sa * x0) + bf(so * noise)), x0 also stored = the training target;
//        mode 1: out = bf(bf(sa * noise_arg) - bf(so * sample)) = get_velocity(sample, noise_arg)).
// sa / so are sqrt(alphas_cumprod[t]) / sqrt(1 - alphas_cumprod[t]) per sample, already rounded to bf16 by the host exactly as the
// scheduler does (it casts alphas_cumprod to the sample dtype first); every product / sum is one bf16 torch op in the reference.
__global__ __launch_bounds__(256) void ddim_mix_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, const float* __restrict__ sa,
                                                       const float* __restrict__ so, float scale, bf16_t* __restrict__ x0_out,
                                                       bf16_t* __restrict__ out, long per_sample, int mode) {
    const int bi = blockIdx.y;
    const float ca = sa[bi], co = so[bi];
    const long base = (long)bi * per_sample;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < per_sample; i += (long)gridDim.x * blockDim.x * 8) {
        float av[8], bv[8], o[8], x0[8];
        unpack8(*reinterpret_cast<const s16x8*>(a + base + i), av);
        unpack8(*reinterpret_cast<const s16x8*>(b + base + i), bv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (mode == 0) {
                x0[e] = rbf(av[e] * scale);
                o[e] = rbf(ca * x0[e]) + rbf(co * bv[e]);
            } else {
                o[e] = rbf(ca * bv[e]) - rbf(co * av[e]);
            }
        }
        *reinterpret_cast<s16x8*>(out + base + i) = pack8(o);
        if (mode == 0 && x0_out) *reinterpret_cast<s16x8*>(x0_out + base + i) = pack8(x0);
    }
}
int ddim_mix(const bf16_t* a, const bf16_t* b, const float* sa, const float* so, float scale, bf16_t* x0_out, bf16_t* out, int B, long per_sample,
             int mode, hipStream_t st) {
    if (per_sample % 8) return set_error(FTMI_ERR_UNSUPPORTED, "ddim_mix: elements per sample must be a multiple of 8");
    if (B <= 0 || per_sample <= 0) return 0;
    long blocks = (per_sample / 8 + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(ddim_mix_kernel, dim3((unsigned)blocks, B), dim3(256), 0, st, a, b, sa, so, scale, x0_out, out, per_sample, mode);
    return check_launch("ddim_mix");
}

// ---------------------------------------------------------------------------------------------------
// Precomputed-latent path (trainer.py:374: --enable_precomputation => compute_posterior = False): the stored "latents" are the VAE's
// posterior moments [B, 2C, ...] = (mean | logvar) and every step draws  x = mean + exp(0.5 * clamp(logvar, -30, 20)) * eps
// (base_specification.py:285-289 -> [upstream] diffusers DiagonalGaussianDistribution.sample), one bf16 torch op at a time.
__global__ __launch_bounds__(256) void posterior_sample_kernel(const bf16_t* __restrict__ moments, const bf16_t* __restrict__ eps,
                                                               bf16_t* __restrict__ out, long half) {
    const int bi = blockIdx.y;
    const bf16_t* mean = moments + (long)bi * 2 * half;
    const bf16_t* logvar = mean + half;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < half; i += (long)gridDim.x * blockDim.x * 8) {
        float mv[8], lv[8], ev[8], o[8];
        unpack8(*reinterpret_cast<const s16x8*>(mean + i), mv);
        unpack8(*reinterpret_cast<const s16x8*>(logvar + i), lv);
        unpack8(*reinterpret_cast<const s16x8*>(eps + (long)bi * half + i), ev);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float l = fminf(fmaxf(lv[e], -30.0f), 20.0f);
            const float sd = rbf(expf(rbf(0.5f * l)));
            o[e] = mv[e] + rbf(sd * ev[e]);
        }
        *reinterpret_cast<s16x8*>(out + (long)bi * half + i) = pack8(o);
    }
}
int posterior_sample(const bf16_t* moments, const bf16_t* eps, bf16_t* out, int B, long half, hipStream_t st) {
    if (half % 8) return set_error(FTMI_ERR_UNSUPPORTED, "posterior_sample: elements per sample must be a multiple of 8");
    if (B <= 0 || half <= 0) return 0;
    long blocks = (half / 8 + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(posterior_sample_kernel, dim3((unsigned)blocks, B), dim3(256), 0, st, moments, eps, out, half);
    return check_launch("posterior_sample");
}

// ---------------------------------------------------------------------------------------------------
// transposes (LoRA working copies; frozen-weight transposes for dgrad are made once at load time)
template <typename TIN>
__global__ __launch_bounds__(256) void transpose_cast_kernel(const TIN* __restrict__ in, bf16_t* __restrict__ out_same, bf16_t* __restrict__ out_t,
                                                             int rows, int cols, long in_bstride, long same_bstride, long t_bstride) {
    __shared__ bf16_t tile[32][33];
    in += (long)blockIdx.z * in_bstride;
    if (out_same) out_same += (long)blockIdx.z * same_bstride;
    out_t += (long)blockIdx.z * t_bstride;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        bf16_t v = 0;
        if (r < rows && c < cols) {
            if constexpr (sizeof(TIN) == 4)
                v = f2bf((float)in[(long)r * cols + c]);
            else
                v = (bf16_t)in[(long)r * cols + c];
            if (out_same) out_same[(long)r * cols + c] = v;
        }
        tile[i][tx] = v;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (r < rows && c < cols) out_t[(long)c * rows + r] = tile[tx][i];
    }
}
// fp32 LoRA matrices -> bf16 (hi, lo) working copies for the fp32-equivalent LoRA branch (LoraSplitArgs, kernels.h).
// One 32 x 32 tile per workgroup; the transposed layouts go through LDS so that every store instruction writes 64-byte runs.
__global__ __launch_bounds__(256) void lora_split_kernel(LoraSplitArgs a) {
    __shared__ uint32_t tile[32][33];  // (hi | lo << 16) of element [i][j]
    const int m = blockIdx.z;
    const int outer = a.inner_n > 0 ? m / a.inner_n : m, inner = a.inner_n > 0 ? m % a.inner_n : 0;
    const float* in = a.w + (long)outer * a.in_bstride + (long)inner * a.in_istride;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    bf16_t* sp = a.sp ? a.sp + (long)outer * a.sp_bstride : nullptr;
    bf16_t* ext = a.ext ? a.ext + (long)outer * a.ext_bstride : nullptr;
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        uint32_t pk = 0;
        if (r < a.rows && c < a.cols) {
            const float v = in[(long)r * a.cols + c];
            const bf16_t hi = f2bf(v), lo = f2bf(v - bf2f(hi));
            pk = (uint32_t)hi | ((uint32_t)lo << 16);
            if (sp) {  // rows interleaved in groups of 32: [hi rows 32g..32g+31 | lo rows 32g..32g+31]
                const long row_hi = (long)(r >> 5) * 64 + (r & 31);
                sp[row_hi * a.cols + c] = hi;
                sp[(row_hi + 32) * a.cols + c] = lo;
            }
            if (ext) {
                bf16_t* e = ext + (long)r * a.ld_ext + c;
                e[0] = hi;
                e[a.cols] = hi;
                e[2 * a.cols] = lo;
            }
        }
        tile[i][tx] = pk;
    }
    if (!a.t_sp && !a.t_ext) return;
    __syncthreads();
    bf16_t* t_sp = a.t_sp ? a.t_sp + (long)outer * a.t_sp_bstride : nullptr;
    bf16_t* t_ext = a.t_ext ? a.t_ext + (long)outer * a.t_ext_bstride + (long)inner * a.t_ext_istride : nullptr;
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;  // element [r][c] of W = element [c][r] of W^T
        if (r < a.rows && c < a.cols) {
            const uint32_t pk = tile[tx][i];
            const bf16_t hi = (bf16_t)(pk & 0xffff), lo = (bf16_t)(pk >> 16);
            if (t_sp) {
                const long row_hi = (long)(c >> 5) * 64 + (c & 31);
                t_sp[row_hi * a.rows + r] = hi;
                t_sp[(row_hi + 32) * a.rows + r] = lo;
            }
            if (t_ext) {
                bf16_t* e = t_ext + (long)c * a.ld_t_ext + r;
                e[0] = hi;
                e[a.rows] = hi;
                e[2 * a.rows] = lo;
            }
        }
    }
}
int lora_split(const LoraSplitArgs& a, hipStream_t st) {
    if (a.rows <= 0 || a.cols <= 0 || a.nmat <= 0) return 0;
    if ((a.sp && a.rows % 32) || (a.t_sp && a.cols % 32)) return set_error(FTMI_ERR_UNSUPPORTED, "lora_split: interleaved planes need multiples of 32 rows");
    dim3 grid((a.cols + 31) / 32, (a.rows + 31) / 32, a.nmat);
    hipLaunchKernelGGL(lora_split_kernel, grid, dim3(256), 0, st, a);
    return check_launch("lora_split");
}
int transpose_bf16(const bf16_t* in, bf16_t* out, int rows, int cols, hipStream_t st) {
    if (rows <= 0 || cols <= 0) return 0;
    dim3 grid((cols + 31) / 32, (rows + 31) / 32, 1);
    hipLaunchKernelGGL(transpose_cast_kernel<bf16_t>, grid, dim3(256), 0, st, in, (bf16_t*)nullptr, out, rows, cols, 0L, 0L, 0L);
    return check_launch("transpose_bf16");
}

// g = bf16(gelu_tanh(z)) from the stashed pre-activation of a GELU GEMM (rows x width, row strides ldz / ldg).  Both GEMM families round z to bf16 first and
// compute the activation from the rounded value with gelu_tanh_f, so this reproduces the g they wrote next to z bit for bit: the LTX backward refills its shared
// g scratch with it instead of keeping 88 MB of g per block.  One 16-byte vector (8 elements) per thread and trip; the width % 8 tail of a row, and every element
// when a base or a stride breaks the 16-byte alignment, goes through the scalar loop.  Nothing outside the rows x width window is read or written.
__global__ __launch_bounds__(256) void gelu_from_pre_kernel(const bf16_t* __restrict__ z, long ldz, bf16_t* __restrict__ g, long ldg, int rows, int width, int vec) {
    const int nv = vec ? width >> 3 : 0;  // whole vectors per row
    const long nvec = (long)rows * nv;
    const long stride = (long)gridDim.x * blockDim.x;
    const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long i = t0; i < nvec; i += stride) {
        const long r = i / nv;
        const int c = (int)(i - r * nv) << 3;
        const u32x4 in = *reinterpret_cast<const u32x4*>(z + r * ldz + c);
        u32x4 out;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = gelu_tanh_f(bf2f((bf16_t)(in[j] & 0xffff)));
            const float b = gelu_tanh_f(bf2f((bf16_t)(in[j] >> 16)));
            out[j] = pack2bf(a, b);
        }
        *reinterpret_cast<u32x4*>(g + r * ldg + c) = out;
    }
    const int tail0 = nv << 3, nt = width - tail0;  // scalar columns [tail0, width) of every row
    const long ntail = (long)rows * nt;
    for (long i = t0; i < ntail; i += stride) {
        const long r = i / nt;
        const int c = tail0 + (int)(i - r * nt);
        g[r * ldg + c] = f2bf(gelu_tanh_f(bf2f(z[r * ldz + c])));
    }
}
int gelu_from_pre(const bf16_t* z, long ldz, bf16_t* g, long ldg, int rows, int width, hipStream_t st) {
    if (rows <= 0 || width <= 0) return 0;
    if (!z || !g || ldz < width || ldg < width) return set_error(FTMI_ERR_INVALID, "gelu_from_pre: null tensor or a row stride below the width");
    const int vec = ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(g)) % 16 == 0) && ldz % 8 == 0 && ldg % 8 == 0;
    const long work = vec ? (long)rows * ((width + 7) / 8) : (long)rows * width;
    long blocks = (work + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;  // 16 workgroups of 4 waves per CU, grid-stride beyond
    hipLaunchKernelGGL(gelu_from_pre_kernel, dim3((unsigned)blocks), dim3(256), 0, st, z, ldz, g, ldg, rows, width, vec);
    return check_launch("gelu_from_pre");
}

}  // namespace ftmi
