// What the step kernels of the three latent samplers share (ltx_sample.hip: cfg_euler_step; sample_layout.hip: wan_sample_step, cog_sample_step): a
// thread owns vector i of 8 consecutive elements, reads 16 bytes of each half of pred, combines them in fp32 --
//       d = c - u;   v = fma(g, d, u)                                                              (guidance == 1: v = c, no unconditional half)
// -- applies its model's own update line to x, and stores bf16(x) (round to nearest even) to the one or two row groups of the next model input.
#pragma once
#include "common.hip.h"

namespace ftmi {

FTMI_DEVICE void unpack8(const u32x4& p, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(p[i] << 16);
        f[2 * i + 1] = __uint_as_float(p[i] & 0xffff0000u);
    }
}

// v[8] of vector i of pred bf16 [2, n8 vectors] (kCfg: rows [0, n8) unconditional, [n8, 2 n8) conditional) or [n8 vectors]
template <bool kCfg>
FTMI_DEVICE void cfg_combine8(const bf16_t* __restrict__ pred, long i, long n8, float g, float* v) {
    const u32x4* pp = reinterpret_cast<const u32x4*>(pred);
    if (kCfg) {
        float u[8], c[8];
        unpack8(pp[i], u);
        unpack8(pp[n8 + i], c);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaf(g, c[e] - u[e], u[e]);
    } else {
        unpack8(pp[i], v);
    }
}

// bf16(xv[8]) as one 16-byte vector at element `at` of cols, and (kCfg) again `group` elements further: the second row group
template <bool kCfg>
FTMI_DEVICE void store_groups8(bf16_t* __restrict__ cols, const float* xv, long at, long group) {
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack2bf(xv[2 * e], xv[2 * e + 1]);
    *reinterpret_cast<u32x4*>(cols + at) = o;
    if (kCfg) *reinterpret_cast<u32x4*>(cols + at + group) = o;
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace ftmi
