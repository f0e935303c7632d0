// Inference-only attention forward on the 8-bit matrix instructions of gfx950: S^T = K8.Q8^T on v_mfma_i32_32x32x32_i8, O^T = V8^T.P8^T on
// v_mfma_f32_32x32x64_f8f6f4 (e4m3 x e4m3, fp32 accumulation), behind a row-wise quantising pre-pass.  head_dim 64 and 128, any Sq >= 1, any Sk >= 1, optional
// additive key bias (-inf removes a key), bf16 output, no lse.  Reference site: the sage providers of finetrainers/models/attention_dispatch.py:1651-1760
// (SageAttention: int8 Q / K with K smoothing, fp8 P / V), which exist for CUDA only.
//
// Pre-pass (two launches, memory-bound; q8_stats_kernel, q8_quant_kernel) into a caller-owned workspace, every piece rounded up to 256 bytes, in this order:
//   q8    int8  [B, H, Sq, d]         codes of plain Q, one scale per ROW (a lane of the transposed product owns one query row, so the finer scale costs one
//   sq    fp32  [B, H, Sq]            scalar per lane; Sage scales per block).  softmax scale * log2 e is NOT folded in: the forward multiplies it onto sq once.
//   k8    int8  [B, H, nt, 64 d]      nt = ceil(Sk / 64) tile IMAGES (below) of K - mean_keys(K): the per-(b, h, channel) mean over the Sk keys, in fp32,
//   sk    fp32  [B, H, nt]            is Sage's K smoothing (it adds the same q.mean to every logit of a row: softmax does not see it); smooth_k = 0 skips it.
//                                     One scale per 64-key tile.
//   v8    e4m3  [B, H, nt, d 64]      tile images of V / sv, sv = absmax_keys |V| / 448 per (b, h, channel): V on the full e4m3 range, as SageAttention2 does
//   sv    fp32  [B, H, d]
//   ksum  fp32  [B, H, nc, d]         nc = ceil(Sk / 256): column sums of K and column maxima of |V| per 256 keys (q8_stats_kernel), summed in chunk order by
//   vmax  fp32  [B, H, nc, d]         every K / V tile's workgroup: no float atomics, the codes are the same bits on every run
//   Codes: c = rint(x / s) with s = absmax / 127, then one correction step on the exact residual fma(-c, s, x), so |x - c s| <= s / 2 up to the fma's own
//   rounding whatever the division did; a group's largest |code| is 127.  Padded keys of the last tile have code 0 in k8 and v8.
//
// Tile images: the pre-pass owns the layout, so it writes each 64-key tile the way the forward's LDS reads want it and the forward's staging is a LINEAR copy
// (ND = d / 64 direct-to-LDS wave loads of 1 KiB per image and wave, lane l moves bytes 16 l .. 16 l + 15; no per-lane source swizzle, no clamp: the images
// are padded).  16-byte piece `chunk` of row `row` of an image with rows of `pitch` bytes sits at row * pitch + ((chunk ^ f(row)) << 4), f = (row >> 1) & 7 at
// pitch 128 and (row >> 2) & 3 at pitch 64: the ds_read_b128 of 16 lanes on 16 consecutive rows at one chunk takes 16 distinct 16-byte columns of the 256-byte
// bank row (pitch 128: common.hip.h's lds_rm_off; pitch 64: 4 rows per bank row, (row & 3, chunk ^ (row >> 2) & 3) all distinct).
//   K image [64 keys][d bytes]: lane (key = lane & 31, g = lane >> 5) reads piece 2 c + g of row 32 js + key: the A operand of reduction step c (32 channels).
//   V image [d rows][64 bytes], TRANSPOSED: row = channel, and the 64 keys of the tile in the order in which the score tile's C-layout registers become the B
//   operand -- byte 32 g + 16 js + r holds key 32 js + crow(r, g).  Lane (channel = lane & 31, g) reads pieces 2 g, 2 g + 1 of row 32 dt + channel: its 32
//   reduction bytes, two contiguous 16-byte reads and no transposing read.  The reduction index inside an MFMA is a dummy (common.hip.h): byte e of the A lane
//   of half g meets byte e of the B lane of half g -- measured for both instructions, with the C layout of the bf16 form, by tools/probe_mfma8.hip.
//
// Forward (attn_fwd_q8_kernel): 128 queries per workgroup, 32 per wave, Q8 fragments (d / 2 bytes per lane) and sq in registers; workgroup order by XCD as in
// attn_carry.hip.
//   * Score product: 2 x d / 32 int8 MFMAs per 64-key tile into i32 (|sum| <= 127^2 d < 2^24: exact, and exact in v_cvt_f32_i32); dequantisation is ONE
//     multiply by f = (sq[row] scale log2 e) * sk[tile] -- a per-lane scalar times a wave-uniform scalar -- in the conversion to fp32.
//   * What the freed LDS buys: a slot (K image + V image) is 8 KiB (d = 64) / 16 KiB (d = 128), half the bf16 forward's, so THREE slots fit where it has two
//     (25.0 / 49.3 KiB per workgroup, two workgroups per CU as before): tiles t + 1 and t + 2 are in flight under tile t, one counted wait (the loads of
//     tile t + 2 may still fly) and one barrier per tile.  The byte tiles halve the MFMA time per tile, so the same latency needs twice the tiles in flight.
//     The key bias row of a tile rides the same ring (one global_load_lds_dword of wave 0, source index clamped to Sk - 1).
//   * P quantisation: p = exp2(x - m) * 448 -> e4m3 by v_cvt_pk_fp8_f32 in registers (four per register, in C-layout order = the order the V image was written
//     in).  448 is e4m3's largest number and p <= 1, so nothing saturates; the factor is undone EXACTLY because numerator and denominator both carry it (below).
//   * Strict running max, not the bf16 forward's lazy one.  e4m3's smallest subnormal is 2^-9 and rounding is to nearest even, so a weight survives iff
//     p * 448 > 2^-10: the floor is 2^-10 / 448 = 2^-18.8 of the row's current maximum.  A max lagging by up to 2^8 (the bf16 forward) would lift that floor
//     to 2^-10.8, and a tail of 2^12 keys at 2^-12 each -- as much mass as the peak -- would vanish.  With m = the true running max the floor stays below the
//     2^-13 that such a tail needs.  The accumulator rescale is still skipped on every tile where no row of the wave raised its max (one ballot), which after
//     the first tiles is almost every tile; p <= 1 needs x - m <= 0 EXACTLY at the max, so x is rounded once (cvt * f) and m is a max of those same floats.
//   * PV product: 2 ND fp8 MFMAs (K = 64: the whole tile in one instruction per 32 channels) with fp32 accumulation.  CDNA4's MFMA accumulates in fp32, so
//     Sage's two-level accumulation (fp32 partial sums flushed into a second fp32 accumulator, a work-around for the reduced-precision fp8 accumulators of the
//     hardware it targets) is not needed.  sv[channel] is applied once, with 1 / l, at the store.
//   * Row sum: of the QUANTISED P, on the matrix pipe (an all-ones A operand, e4m3 1.0 = 0x38), so o = sv * sum(p8 v8) / sum(p8): the normalised weights sum
//     to one exactly, the factor 448 cancels, and the part of P's rounding that is common to numerator and denominator cancels too.
//   * A row whose keys are all removed (-inf) has no softmax; its output is 0 (l = 0), not NaN.
//   * Registers / LDS (-Rpass-analysis=kernel-resource-usage): DESIGN 7-AB; no scratch in any instance.
#include <cstdio>

#include "common.hip.h"
#include "kernels.h"

namespace ftmi {

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) int i32x16;

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kSlots = 3;
constexpr int kStatKeys = 256;  // keys per partial of q8_stats_kernel
constexpr int q8_lds_bytes(int nd) { return kSlots * 8192 * nd + kSlots * 256 + 256 * nd; }  // ring + key-bias ring + sv

template <int PITCH>
FTMI_DEVICE int img_off(int row, int chunk) {
    const int f = PITCH == 128 ? (row >> 1) & 7 : (row >> 2) & 3;
    return row * PITCH + ((chunk ^ f) << 4);
}

// ---- pre-pass ---------------------------------------------------------------------------------------------------------------------------------------
struct Q8Ws {
    int8_t* q8;
    float* sq;
    uint8_t* k8;
    float* sk;
    uint8_t* v8;
    float* sv;
    float* ksum;
    float* vmax;
    int nt, nc;
};

// column sums of K and column maxima of |V| over the 256 keys of chunk blockIdx.x of (b, h) = blockIdx.y.  A thread owns one 16-byte piece column and every
// RPP-th row; the RPP partials of a channel are added in row order by one thread: a fixed order.
template <int ND>
__global__ __launch_bounds__(256) void q8_stats_kernel(AttnArgs a, Q8Ws w) {
    constexpr int D = 64 * ND, PPR = 8 * ND, RPP = 256 / PPR;
    __shared__ float ss[RPP][D], sm[RPP][D];
    const int tid = threadIdx.x, piece = tid % PPR, r0 = tid / PPR;
    const int chunk = blockIdx.x, bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
    const bf16_t* kb = a.k + (long)b * a.k_sb + (long)h * a.k_sh + piece * 8;
    const bf16_t* vb = a.v + (long)b * a.v_sb + (long)h * a.v_sh + piece * 8;
    float s[8], m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = m[j] = 0.f;
    for (int r = r0; r < kStatKeys; r += RPP) {
        const int key = chunk * kStatKeys + r;
        if (key < a.Sk) {
            const s16x8 kv = *reinterpret_cast<const s16x8*>(kb + (long)key * a.k_ss);
            const s16x8 vv = *reinterpret_cast<const s16x8*>(vb + (long)key * a.v_ss);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                s[j] += bf2f((bf16_t)kv[j]);
                m[j] = fmaxf(m[j], fabsf(bf2f((bf16_t)vv[j])));
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        ss[r0][piece * 8 + j] = s[j];
        sm[r0][piece * 8 + j] = m[j];
    }
    __syncthreads();
    if (tid < D) {
        float sum = 0.f, mx = 0.f;
        for (int r = 0; r < RPP; ++r) {
            sum += ss[r][tid];
            mx = fmaxf(mx, sm[r][tid]);
        }
        const long at = ((long)bh * w.nc + chunk) * D + tid;
        w.ksum[at] = sum;
        w.vmax[at] = mx;
    }
}

// the int8 code of x at scale s > 0: nearest, then one step on the exact residual, so that a division that is off by an ulp cannot cost half a step
FTMI_DEVICE int q8_code(float x, float s) {
    float c = rintf(x / s);
    const float r = __builtin_fmaf(-c, s, x);
    if (r > 0.5f * s) c += 1.f;
    else if (r < -0.5f * s) c -= 1.f;
    return (int)fminf(fmaxf(c, -127.f), 127.f);
}
FTMI_DEVICE u32x2 q8_pack(const float* x, float s) {
    u32x2 w = {0u, 0u};
    if (s > 0.f) {
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j >> 2] |= (uint32_t)(q8_code(x[j], s) & 0xff) << (8 * (j & 3));
    }
    return w;
}

// blockIdx.x < nqt: 64 rows of Q (row-wise scales).  Otherwise K / V tile t = blockIdx.x - nqt: the statistics of (b, h) from the partials, the K image with
// its tile scale, the V image; both images are built in LDS and leave as whole 16-byte pieces.
template <int ND>
__global__ __launch_bounds__(256) void q8_quant_kernel(AttnArgs a, Q8Ws w, int smooth_k, int nqt) {
    constexpr int D = 64 * ND, PPR = 8 * ND, RPP = 256 / PPR, IMG = 4096 * ND, NP = 2 * ND;  // NP pieces per thread and tile
    __shared__ __attribute__((aligned(16))) uint8_t img[2][IMG];
    __shared__ float mean[D], svl[D], red[4];
    const int tid = threadIdx.x;
    const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
    if ((int)blockIdx.x < nqt) {
        const int piece = tid % PPR, r0 = tid / PPR;
        const bf16_t* qb = a.q + (long)b * a.q_sb + (long)h * a.q_sh + piece * 8;
        for (int r = r0; r < 64; r += RPP) {
            const int row = blockIdx.x * 64 + r;
            const bool valid = row < a.Sq;
            float x[8], am = 0.f;
            s16x8 qv = {};
            if (valid) qv = *reinterpret_cast<const s16x8*>(qb + (long)row * a.q_ss);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                x[j] = bf2f((bf16_t)qv[j]);
                am = fmaxf(am, fabsf(x[j]));
            }
#pragma unroll
            for (int o = PPR / 2; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));  // the PPR lanes of a row are neighbours inside one wave
            const float s = am / 127.f;
            if (valid) {
                *reinterpret_cast<u32x2*>(w.q8 + ((long)bh * a.Sq + row) * D + piece * 8) = q8_pack(x, s);
                if (piece == 0) w.sq[(long)bh * a.Sq + row] = s;
            }
        }
        return;
    }
    const int t = blockIdx.x - nqt;
    if (tid < D) {
        float sum = 0.f, mx = 0.f;
        for (int c = 0; c < w.nc; ++c) {
            const long at = ((long)bh * w.nc + c) * D + tid;
            sum += w.ksum[at];
            mx = fmaxf(mx, w.vmax[at]);
        }
        mean[tid] = smooth_k ? sum / (float)a.Sk : 0.f;
        svl[tid] = mx / 448.f;
        if (t == 0) w.sv[(long)bh * D + tid] = mx / 448.f;
    }
    __syncthreads();
    const bf16_t* kb = a.k + (long)b * a.k_sb + (long)h * a.k_sh;
    const bf16_t* vb = a.v + (long)b * a.v_sb + (long)h * a.v_sh;
    float x[NP][8], am = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int idx = tid + 256 * i, r = idx / PPR, piece = idx % PPR, key = t * 64 + r;
        s16x8 kv = {};
        if (key < a.Sk) kv = *reinterpret_cast<const s16x8*>(kb + (long)key * a.k_ss + piece * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            x[i][j] = key < a.Sk ? bf2f((bf16_t)kv[j]) - mean[piece * 8 + j] : 0.f;
            am = fmaxf(am, fabsf(x[i][j]));
        }
    }
    am = wave_max(am);
    if ((tid & 63) == 0) red[tid >> 6] = am;
    __syncthreads();
    const float s = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) / 127.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int idx = tid + 256 * i, r = idx / PPR, piece = idx % PPR, key = t * 64 + r;
        *reinterpret_cast<u32x2*>(&img[0][img_off<D>(r, piece >> 1) + (piece & 1) * 8]) = q8_pack(x[i], s);
        // V: key r of the tile is register r16 of score sub-tile js in lane group g (r & 31 = crow(r16, g)): byte 32 g + 16 js + r16 of its channel's row
        s16x8 vv = {};
        if (key < a.Sk) vv = *reinterpret_cast<const s16x8*>(vb + (long)key * a.v_ss + piece * 8);
        const int rr = r & 31, js = r >> 5, g = (rr >> 2) & 1, r16 = (rr & 3) + 4 * (rr >> 3);
        float y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float sc = svl[piece * 8 + j];
            y[j] = sc > 0.f ? fminf(fmaxf(bf2f((bf16_t)vv[j]) / sc, -448.f), 448.f) : 0.f;
        }
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) {
            const uint32_t pk = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[2 * j2], y[2 * j2 + 1], 0, false);
            img[1][img_off<64>(piece * 8 + 2 * j2, 2 * g + js) + r16] = (uint8_t)(pk & 0xff);
            img[1][img_off<64>(piece * 8 + 2 * j2 + 1, 2 * g + js) + r16] = (uint8_t)((pk >> 8) & 0xff);
        }
    }
    __syncthreads();
    const long tile = ((long)bh * w.nt + t) * IMG;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const int at = (tid + 256 * i) * 16;
        *reinterpret_cast<u32x4*>(w.k8 + tile + at) = *reinterpret_cast<const u32x4*>(&img[0][at]);
        *reinterpret_cast<u32x4*>(w.v8 + tile + at) = *reinterpret_cast<const u32x4*>(&img[1][at]);
    }
    if (tid == 0) w.sk[(long)bh * w.nt + t] = s;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------------------
struct Q8Fwd {
    int B, H, Sq, Sk, nt;
    const int8_t* q8;
    const float* sq;
    const uint8_t* k8;
    const float* sk;
    const uint8_t* v8;
    const float* sv;
    bf16_t* o;
    long o_sb, o_sh, o_ss;
    const float* kbias;
    long kb_sb, kb_sh;
    float c;  // softmax scale * log2 e
};

// direct-to-LDS wave loads (asm form: common.hip.h says why): lane l writes LDS bytes lds + 16 l .. (dwordx4) / lds + 4 l .. (dword) from base + voff
FTMI_DEVICE void dma16(const void* base, uint32_t voff, char* lds) {
    const uint32_t dst = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(dst), "v"(voff), "s"(base) : "memory", "m0");
}
FTMI_DEVICE void dma4(const void* base, uint32_t voff, char* lds) {
    const uint32_t dst = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2" ::"s"(dst), "v"(voff), "s"(base) : "memory", "m0");
}
// at most N of the wave's vector-memory loads still in flight; they retire in issue order, so everything older than the newest N has landed
template <int N>
FTMI_DEVICE void dma_wait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// A wave-uniform fp32 through the scalar cache.  hipcc reads sk[t] with a VECTOR load (the tile DMA's memory clobber keeps it from proving the location
// unwritten) and parks an s_waitcnt vmcnt(0) behind it -- in the middle of the tile, where that retires the DMA of tiles t + 1 and t + 2 as well.  The scalar
// load counts on lgkmcnt and leaves the ring alone.
FTMI_DEVICE float scalar_load(const float* p) {
    float v;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return v;
}
FTMI_DEVICE void settle(const i32x4& f) { asm volatile("" ::"v"(f)); }

FTMI_DEVICE f32x16 mfma_f8(const i32x8& a, const i32x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);  // formats e4m3 / e4m3, zero scale operands: the unscaled instruction
}

template <int ND, bool HAS_KB>
__global__ __launch_bounds__(256, 2) void attn_fwd_q8_kernel(Q8Fwd a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int D = 64 * ND, IMG = 4096 * ND, SLOT = 2 * IMG, NLOAD = 2 * ND;
    char* const bias_ring = smem + kSlots * SLOT;                              // kSlots x 64 fp32
    float* const svl = reinterpret_cast<float*>(bias_ring + kSlots * 256);     // D fp32
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, g = lane >> 5;
    const int ntile = (a.Sq + 127) / 128, nhb = a.H * a.B;
    int hb, qt;  // as in attn_carry.hip: all query tiles of one (batch, head) on one XCD when H * B is a multiple of 8, so its images come out of that L2 (speed only)
    if ((nhb & 7) == 0) {
        const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
        hb = (idx / ntile) * 8 + xcd;
        qt = idx % ntile;
    } else {
        hb = blockIdx.x / ntile;
        qt = blockIdx.x % ntile;
    }
    const int h = hb % a.H, b = hb / a.H;
    const int i = qt * 128 + wave * 32 + li;
    const int ic = min(i, a.Sq - 1);  // rows past Sq compute a copy of the last row and store nothing
    const int nt = a.nt;

    const int8_t* qrow = a.q8 + ((long)hb * a.Sq + ic) * D + 16 * g;
    i32x4 qf[2 * ND];
#pragma unroll
    for (int c = 0; c < 2 * ND; ++c) qf[c] = *reinterpret_cast<const i32x4*>(qrow + 32 * c);
    const float sqc = a.sq[(long)hb * a.Sq + ic] * a.c;
    if (tid < D) svl[tid] = a.sv[(long)hb * D + tid];

    const uint8_t* k8t = a.k8 + (long)hb * nt * IMG;
    const uint8_t* v8t = a.v8 + (long)hb * nt * IMG;
    const float* skp = a.sk + (long)hb * nt;
    const float* kbias = HAS_KB ? a.kbias + (long)b * a.kb_sb + (long)h * a.kb_sh : nullptr;
    uint32_t voff[ND];
#pragma unroll
    for (int n = 0; n < ND; ++n) voff[n] = (uint32_t)((wave * ND + n) * 1024 + lane * 16);
    auto stage = [&](int t, int slot) {
        char* tb = smem + slot * SLOT;
#pragma unroll
        for (int n = 0; n < ND; ++n) dma16(k8t + (long)t * IMG, voff[n], tb + (wave * ND + n) * 1024);
#pragma unroll
        for (int n = 0; n < ND; ++n) dma16(v8t + (long)t * IMG, voff[n], tb + IMG + (wave * ND + n) * 1024);
        if constexpr (HAS_KB) {
            if (wave == 0) dma4(kbias, (uint32_t)min(t * 64 + lane, a.Sk - 1) * 4u, bias_ring + slot * 256);
        }
    };
    // LDS read offsets inside a slot: K piece 2 c + g of row 32 js + li; V pieces 2 g, 2 g + 1 of row 32 dt + li
    int koff[2][2 * ND], vofs[2 * ND][2];
#pragma unroll
    for (int js = 0; js < 2; ++js)
#pragma unroll
        for (int c = 0; c < 2 * ND; ++c) koff[js][c] = img_off<D>(js * 32 + li, 2 * c + g);
#pragma unroll
    for (int dt = 0; dt < 2 * ND; ++dt)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) vofs[dt][hh] = IMG + img_off<64>(dt * 32 + li, 2 * g + hh);

    stage(0, 0);
    if (nt > 1) stage(1, 1);
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 oacc[2 * ND];
#pragma unroll
    for (int dt = 0; dt < 2 * ND; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
#pragma unroll
    for (int c = 0; c < 2 * ND; ++c) settle(qf[c]);
    i32x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = 0x38383838;  // e4m3 1.0
    if (nt > 1) {
        if (HAS_KB && wave == 0) dma_wait<NLOAD + 1>();
        else dma_wait<NLOAD>();
    } else {
        dma_wait<0>();
    }
    __syncthreads();

    int slot = 0;
    float skt = scalar_load(skp);
    for (int t = 0; t < nt; ++t) {
        const char* ks = smem + slot * SLOT;
        const float* kb = reinterpret_cast<const float*>(bias_ring + slot * 256);
        const bool more = t + 2 < nt;
        if (more) stage(t + 2, slot == 0 ? 2 : slot - 1);
        const float f = sqc * skt;

        i32x16 si[2];
#pragma unroll
        for (int js = 0; js < 2; ++js) {
#pragma unroll
            for (int r = 0; r < 16; ++r) si[js][r] = 0;
#pragma unroll
            for (int c = 0; c < 2 * ND; ++c)
                si[js] = __builtin_amdgcn_mfma_i32_32x32x32_i8(*reinterpret_cast<const i32x4*>(ks + koff[js][c]), qf[c], si[js], 0, 0, 0);
        }
        // scores in the log2 domain, rounded ONCE; register r of sub-tile js holds key 64 t + 32 js + crow(r, g)
        float x[2][16], mx = -INFINITY;
#pragma unroll
        for (int js = 0; js < 2; ++js)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
                if constexpr (HAS_KB) b4 = *reinterpret_cast<const f32x4*>(kb + js * 32 + rq * 8 + 4 * g);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sc = (float)si[js][rq * 4 + j] * f;
                    x[js][rq * 4 + j] = HAS_KB ? __builtin_fmaf(b4[j], kLog2e, sc) : sc;
                }
            }
        if (t == nt - 1) {  // padded keys of a ragged last tile: weight exactly 0
#pragma unroll
            for (int js = 0; js < 2; ++js)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (t * 64 + js * 32 + crow(r, g) >= a.Sk) x[js][r] = -INFINITY;
        }
#pragma unroll
        for (int js = 0; js < 2; ++js)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, x[js][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        // strict running max; the rescale runs only on tiles where some row of the wave raised its max.  A max of -inf (every key so far removed) takes the
        // exponent against 0, so that those keys get exp2(-inf) = 0 and not NaN; a row that did not move multiplies by exp2(0) = 1.
        const float m_new = fmaxf(m_run, mx);
        const float m_eff = (m_new == -INFINITY) ? 0.f : m_new;
        if (__builtin_amdgcn_ballot_w64(m_new > m_run) != 0) {
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_eff);
#pragma unroll
            for (int dt = 0; dt < 2 * ND; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
            l_run *= alpha;
        }
        m_run = m_new;
        i32x8 pw;
#pragma unroll
        for (int js = 0; js < 2; ++js)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float p[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) p[j] = __builtin_amdgcn_exp2f(x[js][rq * 4 + j] - m_eff) * 448.f;
                int wd = __builtin_amdgcn_cvt_pk_fp8_f32(p[0], p[1], 0, false);
                wd = __builtin_amdgcn_cvt_pk_fp8_f32(p[2], p[3], wd, true);
                pw[js * 4 + rq] = wd;
            }
        // P.V and the row sums of the quantised P (all-ones A operand): numerator and denominator use the same numbers
#pragma unroll
        for (int dt = 0; dt < 2 * ND; ++dt) {
            const i32x4 lo = *reinterpret_cast<const i32x4*>(ks + vofs[dt][0]), hi = *reinterpret_cast<const i32x4*>(ks + vofs[dt][1]);
            const i32x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            oacc[dt] = mfma_f8(vf, pw, oacc[dt]);
        }
        f32x16 lsum;
#pragma unroll
        for (int r = 0; r < 16; ++r) lsum[r] = 0.f;
        lsum = mfma_f8(ones, pw, lsum);
        l_run += lsum[0];

        if (t + 1 < nt) skt = scalar_load(skp + t + 1);  // here, where the wave is about to wait anyway
        if (more) {  // tile t + 1 has landed once at most the loads of tile t + 2 are in flight
            if (HAS_KB && wave == 0) dma_wait<NLOAD + 1>();
            else dma_wait<NLOAD>();
        } else {
            dma_wait<0>();
        }
        __syncthreads();  // tile t + 1 visible to every wave, tile t's slot free (after the last tile: the output scratch overlays the ring)
        slot = slot == 2 ? 0 : slot + 1;
    }

    // o = sv * acc / l as whole 128-byte bf16 row pieces, through the wave's 4 KiB scratch (16-byte chunks XOR-swizzled by the row)
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
    char* scr = smem + wave * 4096;
    bf16_t* ob = a.o + (long)b * a.o_sb + (long)h * a.o_sh;
    const int row_base = qt * 128 + wave * 32;
#pragma unroll
    for (int dh = 0; dh < ND; ++dh) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const f32x4 s4 = *reinterpret_cast<const f32x4*>(svl + dh * 64 + dt * 32 + rq * 8 + 4 * g);
                const f32x16& t16 = oacc[2 * dh + dt];
                u32x2 pk;
                pk[0] = pack2bf(t16[rq * 4 + 0] * inv * s4[0], t16[rq * 4 + 1] * inv * s4[1]);
                pk[1] = pack2bf(t16[rq * 4 + 2] * inv * s4[2], t16[rq * 4 + 3] * inv * s4[3]);
                *reinterpret_cast<u32x2*>(scr + li * 128 + (((dt * 4 + rq) ^ (li & 7)) << 4) + 8 * g) = pk;
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = it * 8 + (lane >> 3), chunk = lane & 7;
            const u32x4 wv = *reinterpret_cast<const u32x4*>(scr + row * 128 + ((chunk ^ (row & 7)) << 4));
            if (row_base + row < a.Sq) *reinterpret_cast<u32x4*>(ob + (long)(row_base + row) * a.o_ss + dh * 64 + chunk * 8) = wv;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------------------
struct Q8Plan {
    size_t q8, sq, k8, sk, v8, sv, ksum, vmax, total;
    int nt, nc;
};
Q8Plan q8_plan(int B, int H, int Sq, int Sk, int d) {
    Q8Plan p;
    p.nt = (Sk + 63) / 64;
    p.nc = (Sk + kStatKeys - 1) / kStatKeys;
    const size_t bh = (size_t)B * H;
    Bump bump;
    p.q8 = bump.take(bh * Sq * d);
    p.sq = bump.take(bh * Sq * 4);
    p.k8 = bump.take(bh * p.nt * 64 * d);
    p.sk = bump.take(bh * p.nt * 4);
    p.v8 = bump.take(bh * p.nt * 64 * d);
    p.sv = bump.take(bh * d * 4);
    p.ksum = bump.take(bh * p.nc * d * 4);
    p.vmax = bump.take(bh * p.nc * d * 4);
    p.total = bump.off;
    return p;
}
Q8Ws q8_ws(const Q8Plan& p, void* ws) {
    char* c = static_cast<char*>(ws);
    return Q8Ws{reinterpret_cast<int8_t*>(c + p.q8), reinterpret_cast<float*>(c + p.sq), reinterpret_cast<uint8_t*>(c + p.k8), reinterpret_cast<float*>(c + p.sk),
                reinterpret_cast<uint8_t*>(c + p.v8), reinterpret_cast<float*>(c + p.sv), reinterpret_cast<float*>(c + p.ksum), reinterpret_cast<float*>(c + p.vmax),
                p.nt, p.nc};
}

int q8_refuse_misaligned(const char* who, const char* tensor) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s: base pointer and batch / head / token strides must keep 16-byte alignment", who, tensor);
    return set_error(FTMI_ERR_INVALID, msg);
}
bool q8_bad(const void* p, long sb, long sh, long ss) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0 || (sb % 8) || (sh % 8) || (ss % 8); }

// what both entries refuse, before any launch: head_dim, sizes, null tensors, alignment, the workspace
int q8_refuse(const char* who, const AttnQ8Args& q, bool fwd) {
    const AttnArgs& a = q.a;
    char msg[200];
    if (a.d != 64 && a.d != 128) {
        snprintf(msg, sizeof(msg), "%s: head_dim must be 64 or 128", who);
        return set_error(FTMI_ERR_UNSUPPORTED, msg);
    }
    if (a.B <= 0 || a.H <= 0 || a.Sq <= 0 || a.Sk <= 0) {
        snprintf(msg, sizeof(msg), "%s: empty problem", who);
        return set_error(FTMI_ERR_INVALID, msg);
    }
    if (!a.q || !a.k || !a.v || (fwd && !a.o)) {
        snprintf(msg, sizeof(msg), "%s: null tensor", who);
        return set_error(FTMI_ERR_INVALID, msg);
    }
    if (q8_bad(a.q, a.q_sb, a.q_sh, a.q_ss)) return q8_refuse_misaligned(who, "q");
    if (q8_bad(a.k, a.k_sb, a.k_sh, a.k_ss)) return q8_refuse_misaligned(who, "k");
    if (q8_bad(a.v, a.v_sb, a.v_sh, a.v_ss)) return q8_refuse_misaligned(who, "v");
    if (fwd && q8_bad(a.o, a.o_sb, a.o_sh, a.o_ss)) return q8_refuse_misaligned(who, "out");
    if (!q.ws) {
        snprintf(msg, sizeof(msg), "%s: null workspace (ftmi_attn_q8_workspace_bytes says how large; the caller owns it)", who);
        return set_error(FTMI_ERR_INVALID, msg);
    }
    if (reinterpret_cast<uintptr_t>(q.ws) & 255) {
        snprintf(msg, sizeof(msg), "%s: workspace: base pointer must keep 256-byte alignment", who);
        return set_error(FTMI_ERR_INVALID, msg);
    }
    const size_t need = q8_plan(a.B, a.H, a.Sq, a.Sk, a.d).total;
    if (q.ws_bytes < need) {
        snprintf(msg, sizeof(msg), "%s: workspace of %zu bytes, %zu needed", who, q.ws_bytes, need);
        return set_error(FTMI_ERR_INVALID, msg);
    }
    const long nq = (a.Sq + 63) / 64, nt = (a.Sk + 63) / 64;
    if ((long)((a.Sq + 127) / 128) * a.H * a.B > 0x7fffffffL || (long)a.B * a.H > 65535 || nq + nt > 0x7fffffffL) {
        snprintf(msg, sizeof(msg), "%s: too many workgroups", who);
        return set_error(FTMI_ERR_UNSUPPORTED, msg);
    }
    return 0;
}

template <int ND>
int launch_quant(const AttnQ8Args& q, hipStream_t st) {
    const AttnArgs& a = q.a;
    const Q8Plan p = q8_plan(a.B, a.H, a.Sq, a.Sk, a.d);
    const Q8Ws w = q8_ws(p, q.ws);
    hipLaunchKernelGGL(q8_stats_kernel<ND>, dim3(p.nc, a.B * a.H), dim3(256), 0, st, a, w);
    FTMI_TRY(check_launch("attn_q8_quant (statistics)"));
    const int nqt = (a.Sq + 63) / 64;
    hipLaunchKernelGGL(q8_quant_kernel<ND>, dim3(nqt + p.nt, a.B * a.H), dim3(256), 0, st, a, w, q.smooth_k, nqt);
    return check_launch("attn_q8_quant");
}

template <int ND>
int launch_fwd(const AttnQ8Args& q, hipStream_t st) {
    const AttnArgs& a = q.a;
    const Q8Plan p = q8_plan(a.B, a.H, a.Sq, a.Sk, a.d);
    const Q8Ws w = q8_ws(p, q.ws);
    Q8Fwd f;
    f.B = a.B; f.H = a.H; f.Sq = a.Sq; f.Sk = a.Sk; f.nt = p.nt;
    f.q8 = w.q8; f.sq = w.sq; f.k8 = w.k8; f.sk = w.sk; f.v8 = w.v8; f.sv = w.sv;
    f.o = a.o; f.o_sb = a.o_sb; f.o_sh = a.o_sh; f.o_ss = a.o_ss;
    f.kbias = a.kbias; f.kb_sb = a.kb_sb; f.kb_sh = a.kb_sh;
    f.c = a.scale * kLog2e;
    constexpr int lds = q8_lds_bytes(ND);
    const dim3 grid(((a.Sq + 127) / 128) * a.H * a.B);
    if (a.kbias) hipLaunchKernelGGL((attn_fwd_q8_kernel<ND, true>), grid, dim3(256), lds, st, f);
    else hipLaunchKernelGGL((attn_fwd_q8_kernel<ND, false>), grid, dim3(256), lds, st, f);
    return check_launch("attn_fwd_q8");
}

}  // namespace

size_t attn_q8_workspace_bytes(int B, int H, int Sq, int Sk, int d) {
    if (B <= 0 || H <= 0 || Sq <= 0 || Sk <= 0 || (d != 64 && d != 128)) return 0;
    return q8_plan(B, H, Sq, Sk, d).total;
}

int attn_q8_quant(const AttnQ8Args& q, hipStream_t st) {
    FTMI_TRY(q8_refuse("attn_q8_quant", q, false));
    return q.a.d == 128 ? launch_quant<2>(q, st) : launch_quant<1>(q, st);
}

int attn_fwd_q8(const AttnQ8Args& q, hipStream_t st) {
    FTMI_TRY(q8_refuse("attn_fwd_q8", q, true));
    if (!q.prequantised) FTMI_TRY(q.a.d == 128 ? launch_quant<2>(q, st) : launch_quant<1>(q, st));
    ProfScope prof(PROF_ATTN_FWD, 4.0 * q.a.B * q.a.H * (double)q.a.Sq * q.a.Sk * q.a.d, st);
    return q.a.d == 128 ? launch_fwd<2>(q, st) : launch_fwd<1>(q, st);
}

}  // namespace ftmi
