// Second-context attention of a cross-attention with two key/value sets (Wan image-to-video: attn2 attends to the text tokens AND to the CLIP image
// tokens, two independent softmaxes whose bf16 outputs are summed -- [upstream] diffusers WanAttnProcessor2_0 with added_kv_proj_dim).  head_dim 128,
// any Sq, FEW keys (the 257 image tokens: four full 64-key tiles and a tail of one), forward and dQ.  The first context runs through the ordinary
// attention kernels; these two kernels run after it and fold the sum into their output stage, so no element-wise pass over [B, S, D] is needed:
//   forward   o  = bf(float(o_t)  + float(bf(o_i))),   o_i = softmax(q k_i^T scale) v_i,   lse_i written (log2 domain)
//   dQ        dq = bf(float(dq_t) + float(bf(dq_i))),  dq_i = scale * (P_i o (dP_i - delta_i)) k_i,  dP_i = dO v_i^T
// The image keys and values are frozen in the only caller (no adapter sits on add_k_proj / add_v_proj), so there is no dK / dV kernel.
// delta_i = rowsum(dO o O_i) is NOT read from a saved O_i: the dQ kernel walks the (at most five) key tiles twice and forms it in the first walk as
// sum_j P_ij dP_ij (the same number before O_i's rounding), which saves one [B, S, D] tensor per block for two small extra matrix products per tile.
//
// 128 queries per workgroup, 32 per wave; a wave holds its q (and dO) rows as MFMA operand fragments for the whole kernel.  One [64 key][128] tile of K_i
// and of V_i (32 KiB together) is staged through registers into LDS per step, single-buffered: with five tiles per workgroup the kernel is latency-,
// not bandwidth-bound, and the keys are shared by every workgroup of a (batch, head) out of L2.  Keys past Sk are staged as ZEROS and never read from
// memory, and their probabilities are set to exactly 0 (forward: score -inf; dQ: p = 0, not exp2(0 - lse), which overflows for rows whose real logits
// all sit far below zero).  Fragment layouts: common.hip.h.
//
// Two images in the second context (Wan first/last-frame: 2 x 257 = 514 keys, as many as the text branch) go through the WIDE pair further down,
// attn_ctx2w_*: the same arithmetic with tile t + 1 staged under tile t (two LDS slots, one barrier per tile), up to 640 keys.
#include "common.hip.h"
#include "kernels.h"

namespace ftmi {

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kCtx2Lds = 2 * 16384;  // one K tile + one V tile; the output staging (4 waves x 4 KiB) overlays them

// row fragment (non-reduction index = key row) of a [64 tok][64 d] lds_rt_off image: lane (row, g) reads d = 16 c + 8 g .. +7
FTMI_DEVICE s16x8 row_frag(const char* lds, int row, int c, int g) { return *reinterpret_cast<const s16x8*>(lds + lds_rt_off(row, c * 2 + g)); }
// transposed fragment (non-reduction index = d = dbase + (lane & 31)), reduction over the keys tok0 + {4g..4g+3, 8+4g..8+4g+3}: the order pack_frag packs
FTMI_DEVICE s16x8 tr_frag(const char* lds, int dbase, int tok0, int lane) {
    const int g = lane >> 5;
    return lds_tr_frag(lds, dbase, tok0 + 4 * g, tok0 + 8 + 4 * g, lane);
}
FTMI_DEVICE s16x8 pack_frag(const f32x16& v, int hh) {
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = pack2bf(v[hh * 8 + 2 * e], v[hh * 8 + 2 * e + 1]);
    return __builtin_bit_cast(s16x8, w);
}

// keys [64 t, 64 t + 64) of K and V into LDS: two [64][64] images per tensor (d 0..63 | 64..127); keys >= Sk are zeros (their memory is not touched)
FTMI_DEVICE void stage_tile(char* smem, const bf16_t* kbase, long k_ss, const bf16_t* vbase, long v_ss, int t, int Sk, int tid) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int idx = it * 256 + tid, row = idx >> 4, c16 = idx & 15, j = t * 64 + row;
        u32x4 kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
        if (j < Sk) {
            kv = *reinterpret_cast<const u32x4*>(kbase + (long)j * k_ss + c16 * 8);
            vv = *reinterpret_cast<const u32x4*>(vbase + (long)j * v_ss + c16 * 8);
        }
        const int off = (c16 >> 3) * 8192 + lds_rt_off(row, c16 & 7);
        *reinterpret_cast<u32x4*>(smem + off) = kv;
        *reinterpret_cast<u32x4*>(smem + 16384 + off) = vv;
    }
}

// out = bf(float(add) + float(bf(acc * mul))) for the wave's 32 rows x 128 columns.  acc: C layout, column = the wave's row (lane & 31), register r of acc[dt] =
// d (dt >> 1) * 64 + (dt & 1) * 32 + crow(r, g).  The bf16 rounding of acc * mul happens on the way into the wave's LDS scratch (4 KiB, 16-byte chunks
// XOR-swizzled by the row), from which whole 128-byte row pieces are read back, summed with `add` and stored.  `add` and `out` share row_stride and may be
// the same buffer: a lane reads a 16-byte piece and writes the same piece.  Lanes exchange rows through the scratch, so a wavefront-scope fence separates the
// stores from the loads and one half's loads from the next half's stores (the LDS queue of a wave is in order; the fence keeps the compiler to that order).
FTMI_DEVICE void store_sum_rows(char* scr, const f32x16 (&acc)[4], float mul, const bf16_t* add, bf16_t* out, long row_stride, int row_base, int nrows, int lane) {
    const int li = lane & 31, g = lane >> 5;
#pragma unroll
    for (int dh = 0; dh < 2; ++dh) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const f32x16& t = acc[2 * dh + dt];
                u32x2 pk;
                pk[0] = pack2bf(t[rq * 4 + 0] * mul, t[rq * 4 + 1] * mul);
                pk[1] = pack2bf(t[rq * 4 + 2] * mul, t[rq * 4 + 3] * mul);
                *reinterpret_cast<u32x2*>(scr + li * 128 + (((dt * 4 + rq) ^ (li & 7)) << 4) + 8 * g) = pk;
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = it * 8 + (lane >> 3), chunk = lane & 7;
            const s16x8 w = *reinterpret_cast<const s16x8*>(scr + row * 128 + ((chunk ^ (row & 7)) << 4));
            if (row_base + row < nrows) {
                const long at = (long)(row_base + row) * row_stride + dh * 64 + chunk * 8;
                const s16x8 ad = *reinterpret_cast<const s16x8*>(add + at);
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    o[e] = pack2bf(bf2f((bf16_t)ad[2 * e]) + bf2f((bf16_t)w[2 * e]), bf2f((bf16_t)ad[2 * e + 1]) + bf2f((bf16_t)w[2 * e + 1]));
                *reinterpret_cast<u32x4*>(out + at) = o;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

struct Ctx2Block {
    int tile, h, b;
};
FTMI_DEVICE Ctx2Block ctx2_block(int bid, int ntile, int H) {
    Ctx2Block r;
    const int hb = bid / ntile;
    r.tile = bid % ntile;
    r.h = hb % H;
    r.b = hb / H;
    return r;
}

// ---- forward: a.o = bf(o_t + bf(softmax(q k^T scale) v)), a.lse2 = log2-domain log-sum-exp; o_t has a.o's strides ----------------------------------
__global__ __launch_bounds__(256) void attn_ctx2_fwd_kernel(AttnArgs a, const bf16_t* o_t) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, g = lane >> 5;
    const Ctx2Block blk = ctx2_block(blockIdx.x, (a.Sq + 127) / 128, a.H);
    const int h = blk.h, b = blk.b;
    const int i = blk.tile * 128 + wave * 32 + li;
    const int ic = min(i, a.Sq - 1);
    const float sl = a.scale * kLog2e;

    const bf16_t* qp = a.q + (long)b * a.q_sb + (long)h * a.q_sh + (long)ic * a.q_ss;
    s16x8 qf[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) qf[c] = *reinterpret_cast<const s16x8*>(qp + c * 16 + g * 8);
    const bf16_t* kbase = a.k + (long)b * a.k_sb + (long)h * a.k_sh;
    const bf16_t* vbase = a.v + (long)b * a.v_sb + (long)h * a.v_sh;

    float m_run = -INFINITY, l_run = 0.f;
    f32x16 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;

    const int nt = (a.Sk + 63) / 64;
    const char* ks = smem;
    const char* vs = smem + 16384;
    for (int t = 0; t < nt; ++t) {
        __syncthreads();  // the previous tile's readers are done
        stage_tile(smem, kbase, a.k_ss, vbase, a.v_ss, t, a.Sk, tid);
        __syncthreads();
        f32x16 st[2];
#pragma unroll
        for (int js = 0; js < 2; ++js) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[js][r] = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) st[js] = mfma32(row_frag(ks + (c >> 2) * 8192, js * 32 + li, c & 3, g), qf[c], st[js]);
        }
        if (t == nt - 1) {  // register r of sub-tile js holds key 64 t + 32 js + crow(r, g): padded keys get softmax weight exactly 0
#pragma unroll
            for (int js = 0; js < 2; ++js)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (t * 64 + js * 32 + crow(r, g) >= a.Sk) st[js][r] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int js = 0; js < 2; ++js)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[js][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * sl;  // sl > 0.  Every tile holds at least one real key: mx is finite for finite inputs
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // first tile: exp2(-inf) = 0 on an empty state
        float lval = 0.f;
#pragma unroll
        for (int js = 0; js < 2; ++js)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[js][r] = __builtin_amdgcn_exp2f(st[js][r] * sl - m_new);  // (the product rounded as in mx: the row's largest score gives exactly 1)
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
#pragma unroll
        for (int js = 0; js < 2; ++js)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const s16x8 pf = pack_frag(st[js], hh);
#pragma unroll
                for (int e = 0; e < 8; ++e) lval += bf2f((bf16_t)pf[e]);  // the denominator sums the bf16 probabilities that feed P.V
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) oacc[dt] = mfma32(tr_frag(vs + (dt >> 1) * 8192, (dt & 1) * 32, js * 32 + hh * 16, lane), pf, oacc[dt]);
            }
        lval += __shfl_xor(lval, 32, 64);
        l_run = l_run * alpha + lval;
    }
    __syncthreads();  // the store scratch overlays the tiles
    const long ob = (long)b * a.o_sb + (long)h * a.o_sh;
    store_sum_rows(smem + wave * 4096, oacc, 1.0f / l_run, o_t + ob, a.o + ob, a.o_ss, blk.tile * 128 + wave * 32, a.Sq, lane);
    if (i < a.Sq && g == 0) a.lse2[((long)b * a.H + h) * a.Sq + i] = m_run + __log2f(l_run);
}

// ---- dQ: a.dq = bf(dq_t + bf(scale * (P o (dP - delta)) k)); dq_t has a.dq's strides (and may be a.dq) ----------------------------------------------------
__global__ __launch_bounds__(256) void attn_ctx2_dq_kernel(AttnArgs a, const bf16_t* dq_t) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, g = lane >> 5;
    const Ctx2Block blk = ctx2_block(blockIdx.x, (a.Sq + 127) / 128, a.H);
    const int h = blk.h, b = blk.b;
    const int i = blk.tile * 128 + wave * 32 + li;
    const int ic = min(i, a.Sq - 1);
    const float sl = a.scale * kLog2e;

    const bf16_t* qp = a.q + (long)b * a.q_sb + (long)h * a.q_sh + (long)ic * a.q_ss;
    const bf16_t* dop = a.dout + (long)b * a.do_sb + (long)h * a.do_sh + (long)ic * a.do_ss;
    s16x8 qf[8], dof[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        qf[c] = *reinterpret_cast<const s16x8*>(qp + c * 16 + g * 8);
        dof[c] = *reinterpret_cast<const s16x8*>(dop + c * 16 + g * 8);
    }
    const float lse_i = a.lse2[((long)b * a.H + h) * a.Sq + ic];
    const bf16_t* kbase = a.k + (long)b * a.k_sb + (long)h * a.k_sh;
    const bf16_t* vbase = a.v + (long)b * a.v_sb + (long)h * a.v_sh;

    f32x16 dqt[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dqt[dt][r] = 0.f;

    const int nt = (a.Sk + 63) / 64;
    const char* ks = smem;
    const char* vs = smem + 16384;
    float del_i = 0.f;
    // walk 0: delta = sum_j P_j dP_j;  walk 1: dQ += (P o (dP - delta)) K
    for (int walk = 0; walk < 2; ++walk) {
        for (int t = 0; t < nt; ++t) {
            __syncthreads();
            stage_tile(smem, kbase, a.k_ss, vbase, a.v_ss, t, a.Sk, tid);
            __syncthreads();
#pragma unroll
            for (int js = 0; js < 2; ++js) {
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[r] = 0.f;
                    dp[r] = 0.f;
                }
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    s = mfma32(row_frag(ks + (c >> 2) * 8192, js * 32 + li, c & 3, g), qf[c], s);
                    dp = mfma32(row_frag(vs + (c >> 2) * 8192, js * 32 + li, c & 3, g), dof[c], dp);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool real = t * 64 + js * 32 + crow(r, g) < a.Sk;
                    s[r] = real ? __builtin_amdgcn_exp2f(s[r] * sl - lse_i) : 0.f;  // the forward's rounding of the product; (a padded key's zero score would give exp2(-lse))
                }
                if (walk == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) del_i += s[r] * dp[r];
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) dp[r] = s[r] * (dp[r] - del_i);
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const s16x8 dsf = pack_frag(dp, hh);
#pragma unroll
                        for (int dt = 0; dt < 4; ++dt) dqt[dt] = mfma32(tr_frag(ks + (dt >> 1) * 8192, (dt & 1) * 32, js * 32 + hh * 16, lane), dsf, dqt[dt]);
                    }
                }
            }
        }
        if (walk == 0) del_i += __shfl_xor(del_i, 32, 64);  // the two half-waves hold the two halves of a query's keys
    }
    __syncthreads();
    const long qb = (long)b * a.dq_sb + (long)h * a.dq_sh;
    store_sum_rows(smem + wave * 4096, dqt, a.scale, dq_t + qb, a.dq + qb, a.dq_ss, blk.tile * 128 + wave * 32, a.Sq, lane);
}

// ---- the wide pair (up to 640 keys: two images of 257 tokens, Wan first/last-frame) ---------------------------------------------------------------------
// The same arithmetic in the same order as the two kernels above -- 64-key steps, the same online-softmax updates and rounding points, so that for every Sk
// the narrow pair accepts the results are its bits -- with another staging: two LDS slots of 32 KiB, tile t + 1 of K_i / V_i on its way through registers
// (TileRegs, 32 VGPRs; issued before tile t's products, written to the other slot behind them) and ONE barrier per tile.  A slot is overwritten one whole
// iteration after its last reader passed a barrier.  kTwoSlot = false is the lab build's yardstick (FTMI_EXPERIMENTAL): the same loop with the single-buffered
// staging above, i.e. what lifting the 320-key limit alone would have given (profiles/wan_flf_ctx2.txt).
constexpr int kCtx2wSlot = 2 * 16384;
constexpr int kCtx2wMaxKeys = 640;

struct TileRegs {
    u32x4 k[4], v[4];
};
// stage_tile's element-to-thread mapping, in two halves: global -> registers (keys >= Sk: zeros, their memory is not touched), registers -> LDS slot
FTMI_DEVICE void load_tile(TileRegs& r, const bf16_t* kbase, long k_ss, const bf16_t* vbase, long v_ss, int t, int Sk, int tid) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int idx = it * 256 + tid, row = idx >> 4, c16 = idx & 15, j = t * 64 + row;
        r.k[it] = u32x4{0u, 0u, 0u, 0u};
        r.v[it] = u32x4{0u, 0u, 0u, 0u};
        if (j < Sk) {
            r.k[it] = *reinterpret_cast<const u32x4*>(kbase + (long)j * k_ss + c16 * 8);
            r.v[it] = *reinterpret_cast<const u32x4*>(vbase + (long)j * v_ss + c16 * 8);
        }
    }
}
FTMI_DEVICE void write_tile(char* slot, const TileRegs& r, int tid) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int idx = it * 256 + tid, row = idx >> 4, c16 = idx & 15;
        const int off = (c16 >> 3) * 8192 + lds_rt_off(row, c16 & 7);
        *reinterpret_cast<u32x4*>(slot + off) = r.k[it];
        *reinterpret_cast<u32x4*>(slot + 16384 + off) = r.v[it];
    }
}

template <bool kTwoSlot>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn_ctx2w_fwd_kernel(AttnArgs a, const bf16_t* o_t) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, g = lane >> 5;
    const Ctx2Block blk = ctx2_block(blockIdx.x, (a.Sq + 127) / 128, a.H);
    const int h = blk.h, b = blk.b;
    const int i = blk.tile * 128 + wave * 32 + li;
    const int ic = min(i, a.Sq - 1);
    const float sl = a.scale * kLog2e;

    const bf16_t* qp = a.q + (long)b * a.q_sb + (long)h * a.q_sh + (long)ic * a.q_ss;
    s16x8 qf[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) qf[c] = *reinterpret_cast<const s16x8*>(qp + c * 16 + g * 8);
    const bf16_t* kbase = a.k + (long)b * a.k_sb + (long)h * a.k_sh;
    const bf16_t* vbase = a.v + (long)b * a.v_sb + (long)h * a.v_sh;

    float m_run = -INFINITY, l_run = 0.f;
    f32x16 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;

    const int nt = (a.Sk + 63) / 64;
    TileRegs nx;
    if constexpr (kTwoSlot) {
        load_tile(nx, kbase, a.k_ss, vbase, a.v_ss, 0, a.Sk, tid);
        write_tile(smem, nx, tid);
        __syncthreads();
    }
    for (int t = 0; t < nt; ++t) {
        const char* ks = smem + (kTwoSlot ? (t & 1) * kCtx2wSlot : 0);
        const char* vs = ks + 16384;
        if constexpr (kTwoSlot) {
            if (t + 1 < nt) load_tile(nx, kbase, a.k_ss, vbase, a.v_ss, t + 1, a.Sk, tid);  // in flight under this tile's products
        } else {
            __syncthreads();
            stage_tile(smem, kbase, a.k_ss, vbase, a.v_ss, t, a.Sk, tid);
            __syncthreads();
        }
        f32x16 st[2];
#pragma unroll
        for (int js = 0; js < 2; ++js) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[js][r] = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) st[js] = mfma32(row_frag(ks + (c >> 2) * 8192, js * 32 + li, c & 3, g), qf[c], st[js]);
        }
        if (t == nt - 1) {
#pragma unroll
            for (int js = 0; js < 2; ++js)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (t * 64 + js * 32 + crow(r, g) >= a.Sk) st[js][r] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int js = 0; js < 2; ++js)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[js][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * sl;
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        float lval = 0.f;
#pragma unroll
        for (int js = 0; js < 2; ++js)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[js][r] = __builtin_amdgcn_exp2f(st[js][r] * sl - m_new);
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
#pragma unroll
        for (int js = 0; js < 2; ++js)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const s16x8 pf = pack_frag(st[js], hh);
#pragma unroll
                for (int e = 0; e < 8; ++e) lval += bf2f((bf16_t)pf[e]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) oacc[dt] = mfma32(tr_frag(vs + (dt >> 1) * 8192, (dt & 1) * 32, js * 32 + hh * 16, lane), pf, oacc[dt]);
            }
        lval += __shfl_xor(lval, 32, 64);
        l_run = l_run * alpha + lval;
        if constexpr (kTwoSlot) {
            if (t + 1 < nt) write_tile(smem + ((t + 1) & 1) * kCtx2wSlot, nx, tid);  // the slot tile t - 1 was read from, one barrier ago
            __syncthreads();  // tile t + 1 is visible and tile t's readers are done (after the last tile: the store scratch overlays the tiles)
        }
    }
    if constexpr (!kTwoSlot) __syncthreads();
    const long ob = (long)b * a.o_sb + (long)h * a.o_sh;
    store_sum_rows(smem + wave * 4096, oacc, 1.0f / l_run, o_t + ob, a.o + ob, a.o_ss, blk.tile * 128 + wave * 32, a.Sq, lane);
    if (i < a.Sq && g == 0) a.lse2[((long)b * a.H + h) * a.Sq + i] = m_run + __log2f(l_run);
}

template <bool kTwoSlot>
__global__ __launch_bounds__(256) void attn_ctx2w_dq_kernel(AttnArgs a, const bf16_t* dq_t) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, g = lane >> 5;
    const Ctx2Block blk = ctx2_block(blockIdx.x, (a.Sq + 127) / 128, a.H);
    const int h = blk.h, b = blk.b;
    const int i = blk.tile * 128 + wave * 32 + li;
    const int ic = min(i, a.Sq - 1);
    const float sl = a.scale * kLog2e;

    const bf16_t* qp = a.q + (long)b * a.q_sb + (long)h * a.q_sh + (long)ic * a.q_ss;
    const bf16_t* dop = a.dout + (long)b * a.do_sb + (long)h * a.do_sh + (long)ic * a.do_ss;
    s16x8 qf[8], dof[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        qf[c] = *reinterpret_cast<const s16x8*>(qp + c * 16 + g * 8);
        dof[c] = *reinterpret_cast<const s16x8*>(dop + c * 16 + g * 8);
    }
    const float lse_i = a.lse2[((long)b * a.H + h) * a.Sq + ic];
    const bf16_t* kbase = a.k + (long)b * a.k_sb + (long)h * a.k_sh;
    const bf16_t* vbase = a.v + (long)b * a.v_sb + (long)h * a.v_sh;

    f32x16 dqt[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dqt[dt][r] = 0.f;

    const int nt = (a.Sk + 63) / 64;
    float del_i = 0.f;
    TileRegs nx;
    if constexpr (kTwoSlot) {
        load_tile(nx, kbase, a.k_ss, vbase, a.v_ss, 0, a.Sk, tid);
        write_tile(smem, nx, tid);
        __syncthreads();
    }
    int step = 0;  // tiles staged so far over both walks: the slot alternates across the walk boundary
    // walk 0: delta = sum_j P_j dP_j;  walk 1: dQ += (P o (dP - delta)) K
    for (int walk = 0; walk < 2; ++walk) {
        for (int t = 0; t < nt; ++t, ++step) {
            const char* ks = smem + (kTwoSlot ? (step & 1) * kCtx2wSlot : 0);
            const char* vs = ks + 16384;
            const bool more = t + 1 < nt || walk == 0;  // tile 0 of walk 1 loads under the last tile of walk 0
            if constexpr (kTwoSlot) {
                if (more) load_tile(nx, kbase, a.k_ss, vbase, a.v_ss, t + 1 < nt ? t + 1 : 0, a.Sk, tid);
            } else {
                __syncthreads();
                stage_tile(smem, kbase, a.k_ss, vbase, a.v_ss, t, a.Sk, tid);
                __syncthreads();
            }
#pragma unroll
            for (int js = 0; js < 2; ++js) {
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[r] = 0.f;
                    dp[r] = 0.f;
                }
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    s = mfma32(row_frag(ks + (c >> 2) * 8192, js * 32 + li, c & 3, g), qf[c], s);
                    dp = mfma32(row_frag(vs + (c >> 2) * 8192, js * 32 + li, c & 3, g), dof[c], dp);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool real = t * 64 + js * 32 + crow(r, g) < a.Sk;
                    s[r] = real ? __builtin_amdgcn_exp2f(s[r] * sl - lse_i) : 0.f;
                }
                if (walk == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) del_i += s[r] * dp[r];
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) dp[r] = s[r] * (dp[r] - del_i);
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const s16x8 dsf = pack_frag(dp, hh);
#pragma unroll
                        for (int dt = 0; dt < 4; ++dt) dqt[dt] = mfma32(tr_frag(ks + (dt >> 1) * 8192, (dt & 1) * 32, js * 32 + hh * 16, lane), dsf, dqt[dt]);
                    }
                }
            }
            if constexpr (kTwoSlot) {
                if (more) write_tile(smem + ((step + 1) & 1) * kCtx2wSlot, nx, tid);
                __syncthreads();
            }
        }
        if (walk == 0) del_i += __shfl_xor(del_i, 32, 64);
    }
    if constexpr (!kTwoSlot) __syncthreads();
    const long qb = (long)b * a.dq_sb + (long)h * a.dq_sh;
    store_sum_rows(smem + wave * 4096, dqt, a.scale, dq_t + qb, a.dq + qb, a.dq_ss, blk.tile * 128 + wave * 32, a.Sq, lane);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool rows8(long sb, long sh, long ss) { return sb % 8 == 0 && sh % 8 == 0 && ss % 8 == 0; }

int check_ctx2(const AttnArgs& a) {
    if (a.d != 128) return set_error(FTMI_ERR_UNSUPPORTED, "attn_ctx2: head_dim must be 128");
    if (a.B < 0 || a.H <= 0 || a.Sq < 0 || a.Sk <= 0) return set_error(FTMI_ERR_INVALID, "attn_ctx2: empty key set or negative size");
    if (a.Sk > 320) return set_error(FTMI_ERR_UNSUPPORTED, "attn_ctx2: at most 320 keys (the second context is the few image tokens; use ftmi_attn_fwd for long contexts)");
    if (!rows8(a.q_sb, a.q_sh, a.q_ss) || !rows8(a.k_sb, a.k_sh, a.k_ss) || !rows8(a.v_sb, a.v_sh, a.v_ss) || !aligned16(a.q) || !aligned16(a.k) || !aligned16(a.v))
        return set_error(FTMI_ERR_INVALID, "attn_ctx2: q / k / v rows must keep 16-byte alignment");
    if ((long)((a.Sq + 127) / 128) * a.H * a.B > 0x7fffffffL) return set_error(FTMI_ERR_UNSUPPORTED, "attn_ctx2: too many workgroups");
    return 0;
}

// the wide pair's refusals: check_ctx2's, with the key range 1 .. 640
int check_ctx2w(const AttnArgs& a) {
    if (a.d != 128) return set_error(FTMI_ERR_UNSUPPORTED, "attn_ctx2w: head_dim must be 128");
    if (a.B < 0 || a.H <= 0 || a.Sq < 0 || a.Sk <= 0) return set_error(FTMI_ERR_INVALID, "attn_ctx2w: empty key set or negative size");
    if (a.Sk > kCtx2wMaxKeys) return set_error(FTMI_ERR_UNSUPPORTED, "attn_ctx2w: at most 640 keys (two images of up to 320 tokens; use ftmi_attn_fwd for long contexts)");
    if (!rows8(a.q_sb, a.q_sh, a.q_ss) || !rows8(a.k_sb, a.k_sh, a.k_ss) || !rows8(a.v_sb, a.v_sh, a.v_ss) || !aligned16(a.q) || !aligned16(a.k) || !aligned16(a.v))
        return set_error(FTMI_ERR_INVALID, "attn_ctx2w: q / k / v rows must keep 16-byte alignment");
    if ((long)((a.Sq + 127) / 128) * a.H * a.B > 0x7fffffffL) return set_error(FTMI_ERR_UNSUPPORTED, "attn_ctx2w: too many workgroups");
    return 0;
}

template <bool kTwoSlot>
int ctx2w_fwd(const AttnArgs& a, const bf16_t* o_t, hipStream_t st) {
    FTMI_TRY(check_ctx2w(a));
    if (!a.q || !a.k || !a.v || !a.o || !a.lse2 || !o_t) return set_error(FTMI_ERR_INVALID, "attn_ctx2w_fwd: null tensor");
    if (!rows8(a.o_sb, a.o_sh, a.o_ss) || !aligned16(a.o) || !aligned16(o_t)) return set_error(FTMI_ERR_INVALID, "attn_ctx2w_fwd: output rows must keep 16-byte alignment");
    if (a.B == 0 || a.Sq == 0) return 0;
    const int grid = ((a.Sq + 127) / 128) * a.H * a.B;
    hipLaunchKernelGGL(attn_ctx2w_fwd_kernel<kTwoSlot>, dim3(grid), dim3(256), kTwoSlot ? 2 * kCtx2wSlot : kCtx2wSlot, st, a, o_t);
    return check_launch("attn_ctx2w_fwd");
}

template <bool kTwoSlot>
int ctx2w_dq(const AttnArgs& a, const bf16_t* dq_t, hipStream_t st) {
    FTMI_TRY(check_ctx2w(a));
    if (!a.q || !a.k || !a.v || !a.lse2 || !a.dout || !a.dq || !dq_t) return set_error(FTMI_ERR_INVALID, "attn_ctx2w_dq: null tensor");
    if (!rows8(a.do_sb, a.do_sh, a.do_ss) || !rows8(a.dq_sb, a.dq_sh, a.dq_ss) || !aligned16(a.dout) || !aligned16(a.dq) || !aligned16(dq_t))
        return set_error(FTMI_ERR_INVALID, "attn_ctx2w_dq: dO / dQ rows must keep 16-byte alignment");
    if (a.B == 0 || a.Sq == 0) return 0;
    const int grid = ((a.Sq + 127) / 128) * a.H * a.B;
    hipLaunchKernelGGL(attn_ctx2w_dq_kernel<kTwoSlot>, dim3(grid), dim3(256), kTwoSlot ? 2 * kCtx2wSlot : kCtx2wSlot, st, a, dq_t);
    return check_launch("attn_ctx2w_dq");
}

}  // namespace

int attn_ctx2w_fwd(const AttnArgs& a, const bf16_t* o_t, hipStream_t st) { return ctx2w_fwd<true>(a, o_t, st); }
int attn_ctx2w_dq(const AttnArgs& a, const bf16_t* dq_t, hipStream_t st) { return ctx2w_dq<true>(a, dq_t, st); }
#ifdef FTMI_EXPERIMENTAL
int attn_ctx2w1_fwd(const AttnArgs& a, const bf16_t* o_t, hipStream_t st) { return ctx2w_fwd<false>(a, o_t, st); }
int attn_ctx2w1_dq(const AttnArgs& a, const bf16_t* dq_t, hipStream_t st) { return ctx2w_dq<false>(a, dq_t, st); }
#endif

int attn_ctx2_fwd(const AttnArgs& a, const bf16_t* o_t, hipStream_t st) {
    FTMI_TRY(check_ctx2(a));
    if (!a.q || !a.k || !a.v || !a.o || !a.lse2 || !o_t) return set_error(FTMI_ERR_INVALID, "attn_ctx2_fwd: null tensor");
    if (!rows8(a.o_sb, a.o_sh, a.o_ss) || !aligned16(a.o) || !aligned16(o_t)) return set_error(FTMI_ERR_INVALID, "attn_ctx2_fwd: output rows must keep 16-byte alignment");
    if (a.B == 0 || a.Sq == 0) return 0;
    const int grid = ((a.Sq + 127) / 128) * a.H * a.B;
    hipLaunchKernelGGL(attn_ctx2_fwd_kernel, dim3(grid), dim3(256), kCtx2Lds, st, a, o_t);
    return check_launch("attn_ctx2_fwd");
}

int attn_ctx2_dq(const AttnArgs& a, const bf16_t* dq_t, hipStream_t st) {
    FTMI_TRY(check_ctx2(a));
    if (!a.q || !a.k || !a.v || !a.lse2 || !a.dout || !a.dq || !dq_t) return set_error(FTMI_ERR_INVALID, "attn_ctx2_dq: null tensor");
    if (!rows8(a.do_sb, a.do_sh, a.do_ss) || !rows8(a.dq_sb, a.dq_sh, a.dq_ss) || !aligned16(a.dout) || !aligned16(a.dq) || !aligned16(dq_t))
        return set_error(FTMI_ERR_INVALID, "attn_ctx2_dq: dO / dQ rows must keep 16-byte alignment");
    if (a.B == 0 || a.Sq == 0) return 0;
    const int grid = ((a.Sq + 127) / 128) * a.H * a.B;
    hipLaunchKernelGGL(attn_ctx2_dq_kernel, dim3(grid), dim3(256), kCtx2Lds, st, a, dq_t);
    return check_launch("attn_ctx2_dq");
}

}  // namespace ftmi
