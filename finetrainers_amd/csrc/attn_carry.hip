// Forward attention that CONTINUES a softmax state carried in fp32 over the next chunk of keys (context parallelism: a rank attends its query shard to the
// key / value chunk of every rank in turn; joint attention over keys that live in two buffers), and the streaming fp32 accumulation of bf16 gradients that
// the chunked backward needs.  n chunks are n launches of attn_fwd_carry_kernel with nothing in between: no bf16 partial output, no merge pass, no rounding
// per chunk.  head_dim 64 and 128, any Sq, any Sk >= 1, optional additive key bias (-inf removes a key).
//
// The state of a query row is (acc = normalised running output, fp32 [d]; lse = running log-sum-exp, log2 domain).  acc * 2^lse is the un-normalised
// numerator, so a row re-enters the online softmax EXACTLY at running max m = lse, running sum l = 1, accumulator = acc, and leaves it as acc = accumulator / l,
// lse = m + log2 l.  Design ("Carried-softmax forward"):
//   * S^T = K.Q^T and O^T = V^T.P^T on v_mfma_f32_32x32x16_bf16, as in attention.hip: a lane owns one query row, so m and l are per-lane scalars and the
//     C-layout registers of P are the B operand of the second product.  128 queries per workgroup, 32 per wave.
//   * The carried accumulator is not a second copy next to the P.V accumulators: it is loaded INTO them.  Register r of accumulator tile dt holds
//     d = 32 dt + crow(r, g), i.e. four consecutive d per group of four registers -- one 16-byte piece of the fp32 row -- so the state is read and written
//     with 2 * d / 16 global_load / store_dwordx4 per lane straight from / to the MFMA registers, no LDS pass and no extra VGPRs (64 accumulator registers at
//     head_dim 128 as in the one-call forward: two workgroups per CU).  The two half-waves of a row cover 32 contiguous bytes per instruction.
//   * The state read is issued BEHIND the first K / V tile's direct-to-LDS loads and retires with them at the one wait in front of the loop.
//   * K / V tiles of 64 keys go global -> LDS directly (common.hip.h: TileDma) into two slots; tile t + 1 is in flight under tile t; one barrier per tile.
//     The last tile clamps its source rows to the view (no read past Sk) and gives the padded keys weight exactly 0.
//   * Lazy rescale as in the one-call forward (the running max moves only when some row of the wave outgrew it by 2^8), row sums on the matrix pipe.
#include <cstdio>
#include <type_traits>

#include "common.hip.h"
#include "kernels.h"

namespace ftmi {

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kCarryLds64 = 2 * 16384 + 2 * 256;  // two (K, V) slots + two key-bias rows; the per-wave output scratch (4 x 4 KiB) overlays slot 0
constexpr int kCarryLds128 = 2 * 32768 + 2 * 256;

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
// hipcc places the wait of an ordinary global load at its first use -- inside the tile loop, where the hardware counter also holds the (inline-asm) tile
// DMA of the next tile.  Consuming the registers in an empty statement before the loop keeps those waits out of it.
FTMI_DEVICE void settle(const s16x8& f) { asm volatile("" ::"v"(f)); }
FTMI_DEVICE void settle(const f32x4& f) { asm volatile("" ::"v"(f)); }

// 1-D grid of ntile * H * B workgroups -> (tile, head, batch); all tiles of one (batch, head) on one XCD when H * B is a multiple of 8, so that its K / V
// chunk is fetched from the fabric once and re-used out of that XCD's L2 (block b is observed to run on XCD b % 8: speed only)
struct CarryBlock {
    int tile, h, b;
};
FTMI_DEVICE CarryBlock carry_block(int bid, int ntile, int H, int B) {
    const int nhb = H * B;
    int hb, tile;
    if ((nhb & 7) == 0) {
        const int xcd = bid & 7, idx = bid >> 3;
        hb = (idx / ntile) * 8 + xcd;
        tile = idx % ntile;
    } else {
        hb = bid / ntile;
        tile = bid % ntile;
    }
    return CarryBlock{tile, hb % H, hb / H};
}

// bf16(t * mul) of the wave's 32 rows x 64 columns as whole 128-byte row pieces: through the wave's 4 KiB LDS scratch (16-byte chunks XOR-swizzled by the
// row).  Lanes exchange rows through the scratch, so wavefront-scope fences keep the compiler to the in-order LDS queue of the wave.
FTMI_DEVICE void store_bf16_rows(char* scr, const f32x16* t, float mul, bf16_t* base, long row_stride, int row_base, int nrows, int lane) {
    const int li = lane & 31, g = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            u32x2 pk;
            pk[0] = pack2bf(t[dt][rq * 4 + 0] * mul, t[dt][rq * 4 + 1] * mul);
            pk[1] = pack2bf(t[dt][rq * 4 + 2] * mul, t[dt][rq * 4 + 3] * mul);
            *reinterpret_cast<u32x2*>(scr + li * 128 + (((dt * 4 + rq) ^ (li & 7)) << 4) + 8 * g) = pk;
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), chunk = lane & 7;
        const u32x4 w = *reinterpret_cast<const u32x4*>(scr + row * 128 + ((chunk ^ (row & 7)) << 4));
        if (row_base + row < nrows) *reinterpret_cast<u32x4*>(base + (long)(row_base + row) * row_stride + chunk * 8) = w;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ND = head_dim / 64.  a.o may be null (no bf16 output: not the last chunk); a.lse2 and acc are the state, read unless `first`.
template <int ND, bool HAS_KB>
__global__ __launch_bounds__(256, 2) void attn_fwd_carry_kernel(AttnArgs a, float* __restrict__ acc, int first) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, g = lane >> 5;
    const CarryBlock blk = carry_block(blockIdx.x, (a.Sq + 127) / 128, a.H, a.B);
    const int h = blk.h, b = blk.b;
    const int i = blk.tile * 128 + wave * 32 + li;
    const int ic = min(i, a.Sq - 1);  // rows past Sq compute a copy of the last row and store nothing
    const float sl = a.scale * kLog2e;

    const bf16_t* qp = a.q + (long)b * a.q_sb + (long)h * a.q_sh + (long)ic * a.q_ss;
    s16x8 qf[4 * ND];
#pragma unroll
    for (int c = 0; c < 4 * ND; ++c) qf[c] = *reinterpret_cast<const s16x8*>(qp + c * 16 + g * 8);

    const bf16_t* kbase = a.k + (long)b * a.k_sb + (long)h * a.k_sh;
    const bf16_t* vbase = a.v + (long)b * a.v_sb + (long)h * a.v_sh;
    const float* kbias = HAS_KB ? a.kbias + (long)b * a.kb_sb + (long)h * a.kb_sh : nullptr;
    const long srow = ((long)b * a.H + h) * a.Sq + ic;  // the row's place in lse; acc row = srow * d
    float* arow = acc + srow * (64 * ND) + 4 * g;       // register group (dt, rq) <-> arow[32 dt + 8 rq .. + 3]

    const int nt = (a.Sk + 63) / 64;
    const TileDma kd = tile_dma_setup(a.k_ss, a.Sk, wave, lane), vd = tile_dma_setup(a.v_ss, a.Sk, wave, lane);
    float kbr = 0.f;
    // tile t into slot `buf`: K and V by DMA (the last tile's rows clamped to the view); the key-bias row (log2 domain, -inf for padded keys) through a register
    auto stage = [&](int t, int buf) {
        char* tb = smem + buf * (16384 * ND);
#pragma unroll
        for (int dh = 0; dh < ND; ++dh) {
            tile_dma_issue(kd, kbase + 64 * dh, a.k_ss, t, t == nt - 1, tb + dh * 8192, wave);
            tile_dma_issue(vd, vbase + 64 * dh, a.v_ss, t, t == nt - 1, tb + (ND + dh) * 8192, wave);
        }
        if constexpr (HAS_KB) {
            if (tid < 64) {
                const int j = t * 64 + tid;
                kbr = (j < a.Sk) ? kbias[j] * kLog2e : -INFINITY;
            }
        }
    };
    auto stage_commit = [&](int buf) {
        if constexpr (HAS_KB) {
            if (tid < 64) reinterpret_cast<float*>(smem + 2 * 16384 * ND)[buf * 64 + tid] = kbr;
        }
    };

    stage(0, 0);
    // the carried state, under the first tile's loads.  A row that has seen no key yet (lse = -inf) starts like a first call: l = 0, accumulator 0
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 oacc[2 * ND];
    if (first) {
#pragma unroll
        for (int dt = 0; dt < 2 * ND; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
    } else {
        f32x4 sv[8 * ND];
#pragma unroll
        for (int n = 0; n < 8 * ND; ++n) sv[n] = *reinterpret_cast<const f32x4*>(arow + 8 * n);
        m_run = a.lse2[srow];
        const bool seen = m_run != -INFINITY;
        l_run = seen ? 1.f : 0.f;
#pragma unroll
        for (int n = 0; n < 8 * ND; ++n) {
#pragma unroll
            for (int j = 0; j < 4; ++j) sv[n][j] = seen ? sv[n][j] : 0.f;
            settle(sv[n]);
#pragma unroll
            for (int j = 0; j < 4; ++j) oacc[n >> 2][(n & 3) * 4 + j] = sv[n][j];
        }
    }
#pragma unroll
    for (int c = 0; c < 4 * ND; ++c) settle(qf[c]);
    s16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (short)0x3F80;  // bf16 1.0
    stage_commit(0);
    tile_dma_wait();
    __syncthreads();

    auto body = [&](int t, auto CUR) {
        constexpr int cur = decltype(CUR)::value;
        const char* ks = smem + cur * (16384 * ND);
        const char* vs = ks + 8192 * ND;
        const float* kb = reinterpret_cast<const float*>(smem + 2 * 16384 * ND) + cur * 64;
        if (t + 1 < nt) stage(t + 1, cur ^ 1);

        f32x16 st[2];
#pragma unroll
        for (int js = 0; js < 2; ++js) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[js][r] = 0.f;
#pragma unroll
            for (int c = 0; c < 4 * ND; ++c) st[js] = mfma32(row_frag(ks + (c >> 2) * 8192, js * 32 + li, c & 3, g), qf[c], st[js]);
        }
        // scores in the log2 domain; register r of sub-tile js holds key 64 t + 32 js + crow(r, g)
        float mx = -INFINITY;
        if constexpr (HAS_KB) {
#pragma unroll
            for (int js = 0; js < 2; ++js)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(kb + js * 32 + rq * 8 + 4 * g);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float x = __builtin_fmaf(st[js][rq * 4 + j], sl, b4[j]);
                        st[js][rq * 4 + j] = x;
                        mx = fmaxf(mx, x);
                    }
                }
        } else {
            if (t == nt - 1) {  // padded keys of a ragged last tile: weight exactly 0
#pragma unroll
                for (int js = 0; js < 2; ++js)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (t * 64 + js * 32 + crow(r, g) >= a.Sk) st[js][r] = -INFINITY;
            }
#pragma unroll
            for (int js = 0; js < 2; ++js)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[js][r]);
            mx *= sl;  // sl > 0
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        // Lazy rescale: the running max stays while no row of the wave outgrew it by more than 2^8 (probabilities at most 2^8: exact in bf16's exponent
        // range).  The comparison is false for mx = -inf (a tile of removed keys) whatever m_run is, and true for a first real key on an empty state.
        // A max of -inf means every key so far was removed: the exponent is then taken against 0, so that those keys get exp2(-inf) = 0, not NaN.
        float m_new = fmaxf(m_run, mx);
        float alpha = 1.0f;
        if (__builtin_amdgcn_ballot_w64((mx - m_run) > 8.0f) == 0) {
            m_new = m_run;
        } else {
            alpha = __builtin_amdgcn_exp2f(m_run - ((m_new == -INFINITY) ? 0.f : m_new));  // an unchanged row: exp2(0) = 1 exactly
#pragma unroll
            for (int dt = 0; dt < 2 * ND; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
        }
        const float m_eff = (m_new == -INFINITY) ? 0.f : m_new;
#pragma unroll
        for (int js = 0; js < 2; ++js)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                st[js][r] = HAS_KB ? __builtin_amdgcn_exp2f(st[js][r] - m_eff) : __builtin_amdgcn_exp2f(__builtin_fmaf(st[js][r], sl, -m_eff));
        m_run = m_new;

        // P.V; the row sums of the bf16-rounded P ride on the matrix pipe (an all-ones A operand), so numerator and denominator use the same numbers
        f32x16 lsum;
#pragma unroll
        for (int r = 0; r < 16; ++r) lsum[r] = 0.f;
#pragma unroll
        for (int js = 0; js < 2; ++js)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const s16x8 pf = pack_frag(st[js], hh);
#pragma unroll
                for (int dt = 0; dt < 2 * ND; ++dt) oacc[dt] = mfma32(tr_frag(vs + (dt >> 1) * 8192, (dt & 1) * 32, js * 32 + hh * 16, lane), pf, oacc[dt]);
                lsum = mfma32(ones, pf, lsum);
            }
        l_run = l_run * alpha + lsum[0];
        if (t + 1 < nt) stage_commit(cur ^ 1);
        tile_dma_wait();
        __syncthreads();  // tile t + 1 landed and tile t's slot is free again (after the last tile: the output scratch overlays slot 0)
    };
    for (int t = 0; t < nt; t += 2) {
        body(t, std::integral_constant<int, 0>{});
        if (t + 1 < nt) body(t + 1, std::integral_constant<int, 1>{});
    }

    // the new state.  l = 0 only where no key has been seen at all (m = -inf, accumulator 0): acc = 0, lse = -inf, no 0 / 0.  l = 1 with an untouched
    // accumulator (every key of the chunk removed): acc * 1 and m + log2 1 are the bits that came in.
    const bool any = l_run > 0.f;
    const float inv = any ? 1.0f / l_run : 0.f;
    if (i < a.Sq) {
#pragma unroll
        for (int n = 0; n < 8 * ND; ++n) {
            f32x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = oacc[n >> 2][(n & 3) * 4 + j] * inv;
            *reinterpret_cast<f32x4*>(arow + 8 * n) = w;
        }
        if (g == 0) a.lse2[srow] = any ? m_run + __log2f(l_run) : -INFINITY;
    }
    if (a.o) {
        bf16_t* ob = a.o + (long)b * a.o_sb + (long)h * a.o_sh;
#pragma unroll
        for (int dh = 0; dh < ND; ++dh) store_bf16_rows(smem + wave * 4096, &oacc[2 * dh], inv, ob + 64 * dh, a.o_ss, blk.tile * 128 + wave * 32, a.Sq, lane);
    }
}

// acc[i] += float(x[i]) over a [B, H, S, d] view; `out` (x's strides; may be x itself: a lane reads a 16-byte piece and writes the same piece) receives
// bf16(acc) when given.  One 16-byte bf16 piece (two 16-byte fp32 pieces) per lane.
__global__ __launch_bounds__(256) void accum_bf16_kernel(float* __restrict__ acc, const bf16_t* x, bf16_t* out, int H, int S, int d8, long sb, long sh, long ss, long npieces) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npieces) return;
    const int c = (int)(p % d8);
    const long row = p / d8;
    const int s = (int)(row % S);
    const long bh = row / S;
    const long at = (bh / H) * sb + (bh % H) * sh + (long)s * ss + c * 8;
    const s16x8 xv = *reinterpret_cast<const s16x8*>(x + at);
    f32x4* ap = reinterpret_cast<f32x4*>(acc + p * 8);
    f32x4 lo = ap[0], hi = ap[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lo[j] += bf2f((bf16_t)xv[j]);
        hi[j] += bf2f((bf16_t)xv[4 + j]);
    }
    ap[0] = lo;
    ap[1] = hi;
    if (out) {
        u32x4 w;
        w[0] = pack2bf(lo[0], lo[1]);
        w[1] = pack2bf(lo[2], lo[3]);
        w[2] = pack2bf(hi[0], hi[1]);
        w[3] = pack2bf(hi[2], hi[3]);
        *reinterpret_cast<u32x4*>(out + at) = w;
    }
}

bool misaligned(const void* p, const long* s) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0 || (s[0] % 8) || (s[1] % 8) || (s[2] % 8); }
int refuse_misaligned(const char* who, const char* tensor) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s: base pointer and batch / head / token strides must keep 16-byte alignment", who, tensor);
    return set_error(FTMI_ERR_INVALID, msg);
}
int check_desc(const ftmi_attn_desc* d) {
    if (!d) return set_error(FTMI_ERR_INVALID, "attention: null descriptor");
    if (d->d != 64 && d->d != 128) return set_error(FTMI_ERR_UNSUPPORTED, "attention: head_dim must be 64 or 128");
    return 0;
}

template <int ND>
int launch_carry(const AttnArgs& a, float* acc, int first, hipStream_t st) {
    constexpr int lds = ND == 2 ? kCarryLds128 : kCarryLds64;
    static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_fwd_carry_kernel<ND, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess &&
                           hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_fwd_carry_kernel<ND, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
    if (!ok) return set_error(FTMI_ERR_LAUNCH, "attn_fwd_carry: cannot raise the dynamic LDS limit");
    const dim3 grid(((a.Sq + 127) / 128) * a.H * a.B);
    if (a.kbias) hipLaunchKernelGGL((attn_fwd_carry_kernel<ND, true>), grid, dim3(256), lds, st, a, acc, first);
    else hipLaunchKernelGGL((attn_fwd_carry_kernel<ND, false>), grid, dim3(256), lds, st, a, acc, first);
    return check_launch("attn_fwd_carry");
}

}  // namespace

}  // namespace ftmi

using namespace ftmi;

extern "C" {

int ftmi_attn_fwd_carry(const ftmi_attn_desc* desc, const void* q, const void* k, const void* v, float* acc, float* lse, void* out, const float* key_bias,
                        int first, ftmi_stream stream) {
    FTMI_TRY(check_desc(desc));
    if (!q || !k || !v) return set_error(FTMI_ERR_INVALID, "ftmi_attn_fwd_carry: null tensor");
    if (!acc || !lse) return set_error(FTMI_ERR_INVALID, "ftmi_attn_fwd_carry: null state (acc and lse carry the softmax between the calls)");
    if (desc->B <= 0 || desc->H <= 0 || desc->Sq <= 0 || desc->Sk <= 0) return set_error(FTMI_ERR_INVALID, "attn_fwd_carry: empty problem");
    if (misaligned(q, desc->q_strides)) return refuse_misaligned("attn_fwd_carry", "q");
    if (misaligned(k, desc->k_strides)) return refuse_misaligned("attn_fwd_carry", "k");
    if (misaligned(v, desc->v_strides)) return refuse_misaligned("attn_fwd_carry", "v");
    if (out && misaligned(out, desc->o_strides)) return refuse_misaligned("attn_fwd_carry", "out");
    if (reinterpret_cast<uintptr_t>(acc) & 15) return set_error(FTMI_ERR_INVALID, "attn_fwd_carry: acc: base pointer must keep 16-byte alignment");
    if ((long)((desc->Sq + 127) / 128) * desc->H * desc->B > 0x7fffffffL) return set_error(FTMI_ERR_UNSUPPORTED, "attn_fwd_carry: too many workgroups");
    AttnArgs a;
    a.d = desc->d;
    a.B = desc->B; a.H = desc->H; a.Sq = desc->Sq; a.Sk = desc->Sk; a.scale = desc->scale;
    a.q = (const bf16_t*)q; a.q_sb = desc->q_strides[0]; a.q_sh = desc->q_strides[1]; a.q_ss = desc->q_strides[2];
    a.k = (const bf16_t*)k; a.k_sb = desc->k_strides[0]; a.k_sh = desc->k_strides[1]; a.k_ss = desc->k_strides[2];
    a.v = (const bf16_t*)v; a.v_sb = desc->v_strides[0]; a.v_sh = desc->v_strides[1]; a.v_ss = desc->v_strides[2];
    a.o = (bf16_t*)out; a.o_sb = desc->o_strides[0]; a.o_sh = desc->o_strides[1]; a.o_ss = desc->o_strides[2];
    a.lse2 = lse;
    a.kbias = key_bias; a.kb_sb = desc->bias_strides[0]; a.kb_sh = desc->bias_strides[1];
    ProfScope prof(PROF_ATTN_FWD, 4.0 * a.B * a.H * (double)a.Sq * a.Sk * a.d, (hipStream_t)stream);
    return a.d == 128 ? launch_carry<2>(a, acc, first, (hipStream_t)stream) : launch_carry<1>(a, acc, first, (hipStream_t)stream);
}

int ftmi_accum_bf16(const ftmi_attn_desc* desc, float* acc, const void* x, void* out, ftmi_stream stream) {
    FTMI_TRY(check_desc(desc));
    if (!acc || !x) return set_error(FTMI_ERR_INVALID, "ftmi_accum_bf16: null tensor");
    if (desc->B <= 0 || desc->H <= 0 || desc->Sq <= 0) return set_error(FTMI_ERR_INVALID, "accum_bf16: empty problem");
    if (misaligned(x, desc->dq_strides)) return refuse_misaligned("accum_bf16", "x");
    if (out && (reinterpret_cast<uintptr_t>(out) & 15)) return refuse_misaligned("accum_bf16", "out");
    if (reinterpret_cast<uintptr_t>(acc) & 15) return set_error(FTMI_ERR_INVALID, "accum_bf16: acc: base pointer must keep 16-byte alignment");
    const int d8 = desc->d / 8;
    const long npieces = (long)desc->B * desc->H * desc->Sq * d8;
    if ((npieces + 255) / 256 > 0x7fffffffL) return set_error(FTMI_ERR_UNSUPPORTED, "accum_bf16: too many workgroups");
    hipLaunchKernelGGL(accum_bf16_kernel, dim3((unsigned)((npieces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, acc, (const bf16_t*)x, (bf16_t*)out, desc->H, desc->Sq,
                       d8, desc->dq_strides[0], desc->dq_strides[1], desc->dq_strides[2], npieces);
    return check_launch("accum_bf16");
}

}  // extern "C"
