// LTX-Video latent sampling, the kernels around the DiT forward of a denoising loop (the orchestrators are ltx_sample / ltx_sample_cond in ltx_dit.hip).
//
// cfg_euler_step: classifier-free-guidance combine + flow-match Euler update of one sampler step, one pass over memory.
//   pred bf16 [2B, n] (rows [0, B) unconditional, [B, 2B) conditional; guidance == 1: [B, n], no unconditional half), state x fp32 [B, n]
//   updated in place, sigma / sigma_next fp32 [B] on the device.  All arithmetic fp32, four roundings per element:
//       d = c - u;   v = fma(g, d, u);   dt = sigma_next - sigma;   x <- fma(dt, v, x)            (guidance == 1: v = c)
//   and the bf16 round-to-nearest-even copy of the new x goes to both halves of the next model input [2B, n] (once for guidance == 1).
//   Restates [upstream] FlowMatchEulerDiscreteScheduler.step (prev = sample + (sigma_next - sigma) * model_output, state kept in fp32) after the
//   pipeline's noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_uncond).
//   Bytes moved per element of x: 16 with guidance (read u 2 + c 2 + x 4, write x 4 + 2 x 2), 12 without (read c 2 + x 4, write x 4 + 2).
//   Pure streaming: 8 elements per thread, every access a 16-byte vector, grid sized from the element count.
//
//   Held prefix (image-to-video sampling, ltx_sample_cond): the first `hold` elements of every sample are conditioning latents.  For them the kernel reads x
//   once and writes its bf16 copy to xin -- no read of pred, no write of x -- and does nothing at all when there is no xin; the other elements take the
//   update above.  Still one streaming pass of 16-byte accesses (hold % 8 == 0).  Restates [upstream, unpinned] LTXImageToVideoPipeline.__call__: the
//   scheduler steps the frames past the conditioning ones only and the conditioning latents are concatenated back unchanged.
//
// frame_timesteps / cond_rows_expand: the per-frame conditioning of that loop.  A model row sees timestep 0 on its first k latent frames and the step's
//   timestep on the others (t * (1 - conditioning_mask)): frame_timesteps writes that vector [G] (G = model rows x frames); cond_rows_expand copies one
//   of TWO embedding rows (row 0: timestep 0, row 1: the live timestep) into each of the G rows of emb [G, D] and temb [G, 6D].
//
// unpack_denorm: the inverse of noise_pack's normalise + pack: x fp32 [B, S, C] -> latents bf16 [B, C, S] = x * std[c] + mean[c]
//   (_denormalize of finetrainers/models/ltx_video/base_specification.py:427-436 with scaling_factor 1: the normalisation there is
//   (latents - mean) * 1 / std).  64 x 64 tiles through the LDS: reads are 16-byte vectors along C, writes 16-byte vectors along S.
//   Bytes moved per element: 4 read + 2 written.
#include "common.hip.h"
#include "kernels.h"
#include "sample_step.hip.h"

namespace ftmi {

namespace {

// n8 = B * per8 vectors of 8 elements; per8 = per_sample / 8.  kCfg: pred has an unconditional half.  pred == nullptr: no update, only the
// bf16 copies of x (the model input of the first step).  kHold: the first hold8 vectors of every sample are held (copied to xin, never updated).
template <bool kCfg, bool kHold>
__global__ __launch_bounds__(256) void cfg_euler_step_kernel(const bf16_t* __restrict__ pred, float* __restrict__ x, const float* __restrict__ sigma,
                                                             const float* __restrict__ sigma_next, long sig_stride, float g, bf16_t* __restrict__ xin,
                                                             long n8, long per8, long hold8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    long b = 0;
    bool held = false;
    if (kHold) {
        b = i / per8;
        held = i - b * per8 < hold8;
        if (held && !xin) return;  // nothing to copy, nothing to update
    }
    f32x4* xp = reinterpret_cast<f32x4*>(x) + 2 * i;
    f32x4 x0 = xp[0], x1 = xp[1];
    float xv[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    if (pred && !held) {
        if (!kHold) b = i / per8;
        const float dt = sigma_next[b * sig_stride] - sigma[b * sig_stride];
        float v[8];
        cfg_combine8<kCfg>(pred, i, n8, g, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = __builtin_fmaf(dt, v[e], xv[e]);
        x0 = f32x4{xv[0], xv[1], xv[2], xv[3]};
        x1 = f32x4{xv[4], xv[5], xv[6], xv[7]};
        xp[0] = x0;
        xp[1] = x1;
    }
    if (xin) store_groups8<kCfg>(xin, xv, 8 * i, 8 * n8);
}

constexpr int kUnpackPitch = 72;  // bf16 elements per LDS row: 144 bytes, keeps the 16-byte reads aligned

__global__ __launch_bounds__(256) void unpack_denorm_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ std_,
                                                            bf16_t* __restrict__ out, int C, int S) {
    __shared__ __attribute__((aligned(16))) bf16_t tile[64][kUnpackPitch];  // [channel][token]
    const int b = blockIdx.z, c0 = blockIdx.y * 64, s0 = blockIdx.x * 64;
    // in: 64 tokens x 16 vectors of 4 channels (C % 4 == 0, so a vector is inside the row or outside it as a whole)
    for (int idx = threadIdx.x; idx < 64 * 16; idx += 256) {
        const int sl = idx >> 4, c4 = (idx & 15) * 4;
        const int c = c0 + c4, s = s0 + sl;
        if (c < C && s < S) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((long)b * S + s) * C + c);
            const f32x4 sd = *reinterpret_cast<const f32x4*>(std_ + c);
            const f32x4 mn = *reinterpret_cast<const f32x4*>(mean + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[c4 + e][sl] = f2bf(v[e] * sd[e] + mn[e]);
        }
    }
    __syncthreads();
    if ((S & 7) == 0) {  // out: 64 channels x 8 vectors of 8 tokens
        for (int idx = threadIdx.x; idx < 64 * 8; idx += 256) {
            const int cl = idx >> 3, s8 = (idx & 7) * 8;
            const int c = c0 + cl, s = s0 + s8;
            if (c < C && s < S)
                *reinterpret_cast<u32x4*>(out + ((long)b * C + c) * S + s) = *reinterpret_cast<const u32x4*>(&tile[cl][s8]);
        }
    } else {  // rows of the output are not 16-byte aligned: element stores
        for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
            const int cl = idx >> 6, sl = idx & 63;
            const int c = c0 + cl, s = s0 + sl;
            if (c < C && s < S) out[((long)b * C + c) * S + s] = tile[cl][sl];
        }
    }
}

__global__ void bcast_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = src[0];
}

// out[g] = (g % F) < k ? 0 : t[0]  for the G = model rows x F modulation groups of one denoising step
__global__ void frame_timesteps_kernel(const float* __restrict__ t, float* __restrict__ out, int G, int F, int k) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < G) out[g] = (g % F) < k ? 0.0f : t[0];
}

// emb [G, D] / temb [G, 6D] <- row (g % F < k ? 0 : 1) of emb2 [2, D] / temb2 [2, 6D]; one 16-byte vector per thread, grid (ceil(7 D / 8 / 256), G)
__global__ __launch_bounds__(256) void cond_rows_expand_kernel(const bf16_t* __restrict__ emb2, const bf16_t* __restrict__ temb2, bf16_t* __restrict__ emb,
                                                               bf16_t* __restrict__ temb, int F, int k, int D) {
    const int g = blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x, d8 = D / 8;
    if (v >= 7 * d8) return;
    const int src = (g % F) < k ? 0 : 1;
    if (v < d8)
        reinterpret_cast<u32x4*>(emb + (long)g * D)[v] = reinterpret_cast<const u32x4*>(emb2 + (long)src * D)[v];
    else
        reinterpret_cast<u32x4*>(temb + (long)g * 6 * D)[v - d8] = reinterpret_cast<const u32x4*>(temb2 + (long)src * 6 * D)[v - d8];
}

}  // namespace

int cfg_euler_step(const bf16_t* pred, float* x, const float* sigma, const float* sigma_next, long sig_stride, float guidance, bf16_t* xin, int B,
                   long per_sample, hipStream_t st, long hold) {
    if (B <= 0 || per_sample <= 0) return set_error(FTMI_ERR_INVALID, "cfg_euler_step: empty problem");
    if (per_sample % 8) return set_error(FTMI_ERR_UNSUPPORTED, "cfg_euler_step: elements per sample must be a multiple of 8 (16-byte vectors)");
    if (hold < 0 || hold > per_sample) return set_error(FTMI_ERR_INVALID, "cfg_euler_step: the held prefix must lie inside the sample");
    if (hold % 8) return set_error(FTMI_ERR_UNSUPPORTED, "cfg_euler_step: the held prefix must be a multiple of 8 elements (16-byte vectors)");
    if (misaligned(pred) || misaligned(x) || misaligned(xin)) return set_error(FTMI_ERR_INVALID, "cfg_euler_step: tensors must be 16-byte aligned");
    const long per8 = per_sample / 8, n8 = per8 * B, hold8 = hold / 8;
    const long blocks = (n8 + 255) / 256;
    if (blocks > 0x7fffffffL) return set_error(FTMI_ERR_UNSUPPORTED, "cfg_euler_step: too many elements for one launch");
#define FTMI_STEP(CFG, HOLD) \
    hipLaunchKernelGGL((cfg_euler_step_kernel<CFG, HOLD>), dim3((unsigned)blocks), dim3(256), 0, st, pred, x, sigma, sigma_next, sig_stride, guidance, xin, n8, per8, hold8)
    if (guidance != 1.0f) {
        if (hold8 > 0) FTMI_STEP(true, true); else FTMI_STEP(true, false);
    } else {
        if (hold8 > 0) FTMI_STEP(false, true); else FTMI_STEP(false, false);
    }
#undef FTMI_STEP
    return check_launch("cfg_euler_step");
}

int frame_timesteps(const float* t, float* out, int G, int F, int k, hipStream_t st) {
    if (G <= 0 || F <= 0 || k < 0 || k > F) return set_error(FTMI_ERR_INVALID, "frame_timesteps: bad argument");
    hipLaunchKernelGGL(frame_timesteps_kernel, dim3((G + 63) / 64), dim3(64), 0, st, t, out, G, F, k);
    return check_launch("frame_timesteps");
}

int cond_rows_expand(const bf16_t* emb2, const bf16_t* temb2, bf16_t* emb, bf16_t* temb, int G, int F, int k, int D, hipStream_t st) {
    if (G <= 0 || G > 65535 || F <= 0 || k < 0 || k > F || D <= 0 || D % 8) return set_error(FTMI_ERR_INVALID, "cond_rows_expand: bad argument");
    hipLaunchKernelGGL(cond_rows_expand_kernel, dim3((7 * (D / 8) + 255) / 256, G), dim3(256), 0, st, emb2, temb2, emb, temb, F, k, D);
    return check_launch("cond_rows_expand");
}

int unpack_denorm(const float* x, const float* mean, const float* std_, bf16_t* out, int B, int C, int S, hipStream_t st) {
    if (B <= 0 || C <= 0 || S <= 0) return set_error(FTMI_ERR_INVALID, "unpack_denorm: empty problem");
    if (C % 4) return set_error(FTMI_ERR_UNSUPPORTED, "unpack_denorm: channel count must be a multiple of 4 (16-byte vectors)");
    if (B > 65535 || (C + 63) / 64 > 65535) return set_error(FTMI_ERR_UNSUPPORTED, "unpack_denorm: batch / channel count too large for one launch");
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)mean | (uintptr_t)std_) & 15) return set_error(FTMI_ERR_INVALID, "unpack_denorm: tensors must be 16-byte aligned");
    dim3 grid((S + 63) / 64, (C + 63) / 64, B);
    hipLaunchKernelGGL(unpack_denorm_kernel, grid, dim3(256), 0, st, x, mean, std_, out, C, S);
    return check_launch("unpack_denorm");
}

int bcast_f32(const float* src, float* dst, int n, hipStream_t st) {
    if (n <= 0 || n > 64) return set_error(FTMI_ERR_INVALID, "bcast_f32: 1..64 values");
    hipLaunchKernelGGL(bcast_f32_kernel, dim3(1), dim3(64), 0, st, src, dst, n);
    return check_launch("bcast_f32");
}

}  // namespace ftmi
