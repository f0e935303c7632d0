// GEMMs whose weight operand is the stored e4m3fn bytes: one 1-byte copy of a frozen weight W8 [N, ldw8] serves the forward and the input gradient, with no
// up-cast launch and no bf16 arena.  The up-cast e4m3 -> bf16 is exact, so both compute what the bf16 kernels compute on fp8_upcast(W8).
//
//   NT-w8 (forward):         out[M, N] = epi( bf(x[M, K] . W8[N, K]^T + bias)  (+ x2[M, K2] . w2[N, K2]^T) )      epi 0: store;  1: out2 = bf(y), out = bf(gelu(out2))
//   NN-w8 (input gradient):  out[M, K] = epi( bf(dy[M, N] . W8[N, K])          (+ x2[M, K2] . w2[K, K2]^T) )      epi 0: store;  3: out = bf(bf(y) gelu'(aux))
//
// Rounding points: ftmi_gemm_nt_ex's (y = bf(product + bias); extension: y = bf(y) + x2 w2^T).  Below R is the reduction depth and C the output width
// (NT: R = K, C = N;  NN: R = N, C = K); `X` is the bf16 activation operand (x / dy).  Reference site: diffusers' layerwise casting (storage float8_e4m3fn,
// compute bf16) around F.linear / peft lora.Linear and autograd's grad_input of it.
//
// Tile (gemm_nn.hip's).  One workgroup (4 waves, 2 x 2) owns 256 rows x 128 output columns and walks R in 64-deep stages; a wave owns 128 rows x 64 columns =
// 4 x 2 MFMA tiles (v_mfma_f32_32x32x16_bf16, A-slot = W fragment, B-slot = X fragment: a lane owns output row m = lane & 31 and, per register quad, 4
// consecutive columns).
//
// Staging.  The bytes travel as bytes.  A stage is four [64][64] bf16 sub-tiles of X (8 KiB each, lds_rt_off images as in gemm_nn.hip) and ONE 8 KiB byte
// sub-tile of W8, all by direct-to-LDS wave loads of 1 KiB (16 bytes per lane, asm form: common.hip.h says why): 10 loads per wave and stage against gemm_nn's
// 12, 40 KiB per slot against 48.  Three slots; one counted wait and one barrier per stage (gemm_nn.hip's argument).  Instances with a K-extension keep
// 48 KiB slots, because an extension stage holds 16 KiB of bf16 w2 where the bytes were (12 loads; the counted wait follows the NEXT stage's kind).
//
// NT byte sub-tile: 128 output rows x 64 bytes (the stage's 64 reduction values of each row), 512 pieces of 16 bytes.  Piece j (0..3) of row r sits at
//   r * 64 + ((j ^ ((r >> 2) & 3)) << 4).
//   DMA: wave load L (0..7) fills rows 16 L .. 16 L + 15, lane l writes LDS byte 1024 L + 16 l (wave-linear, conflict-free by construction) from source row
//   16 L + (l >> 2), piece (l & 3) ^ f(row): the swizzle is on the SOURCE address, every row is still read as one 64-byte line.
//   Read: ds_read_b128 -- lane (c = lane & 31, g = lane >> 5) takes piece 2 p + g of row 32 tn + c: SIXTEEN reduction values, i.e. the W fragments of two
//   MFMA steps (bytes 0-7 and 8-15).  The reduction index inside an MFMA is a dummy (common.hip.h), so step (p, h) pairs them with X chunk 4 p + 2 g + h.  A
//   b128 read is served 16 lanes at a time = 16 consecutive rows r = 4 a + b at one j: 16-byte column (slot mod 16) = 4 b + (j ^ a), all sixteen distinct: the
//   256-byte bank row exactly once, no conflict.  (An 8-byte read per fragment cannot be conflict-free here: the DMA moves 16-byte pieces, a 32-lane pass of a
//   64-bit read has one g, so all 32 lanes would take the same half of their pieces -- 32 lanes on 16 bank pairs.  The 16-byte read also halves the reads.)
//
// NN byte sub-tile: 64 reduction rows x 128 bytes (the tile's 128 output columns), memory layout.  Piece ch (0..7) of row n sits at
//   n * 128 + ((ch ^ (((n >> 1) & 3) << 1)) << 4).
//   DMA: wave load L fills rows 8 L .. 8 L + 7, lane l writes 1024 L + 16 l from source row 8 L + (l >> 3), piece (l & 7) ^ f(row): whole 128-byte lines.
//   Read: ds_read_b64_tr_b8.  Lane map (derived from the b16 form's measured one, then MEASURED: tools/probe_tr8.hip): inside each 16-lane group lane 2 j + q
//   supplies the address of 8 contiguous bytes = R[j][8 q .. 8 q + 7] of an 8 x 16 byte matrix R, and lane c receives column c: (R[0][c], ..., R[7][c]).
//   Group u = lane >> 4 is MFMA column block (u & 1) of k-group g = u >> 1, so lane 2 j + q addresses row 16 kk + 8 g + j, bytes 32 tn + 16 (u & 1) + 8 q ...
//   of the wave's 64, and lane c receives output column 32 tn + 16 (u & 1) + c at reduction rows 16 kk + 8 g + {0..7} -- the n of X chunk 2 kk + g.  ONE read
//   per fragment (the b16 form needs two).  A 32-lane pass (one g) takes 8 consecutive rows x 32 contiguous bytes = pieces (2 a, 2 a + 1) of rows n0 .. n0 + 7:
//   16-byte column = 8 (n & 1) + ((2 a + b) ^ 2 v) = 8 (n & 1) + 2 (a ^ v) + b with v = (n >> 1) & 3: distinct over (n & 1, v, b): the bank row once, no conflict.
//
// Conversion.  8 bytes -> one 8 x bf16 fragment in registers by four v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 (byte 0 of the selected half -> low bf16).
// Measured exact on all 254 non-NaN bytes in every byte position, subnormals included, 0x7f / 0xff -> NaN (tools/probe_tr8.hip).  A fragment is converted
// once per stage step and used for the wave's four row tiles: 8 conversions per 8 MFMAs.
//
// Extension stages, the GELU' epilogue with its early aux request, the 8 rows x 128 bytes store path, 64-bit tile bases with 32-bit per-lane offsets, the
// xcd_remap tile order (row tile fastest: the workgroups of one XCD share a W8 panel) and refusal before launch are gemm_nn.hip's.  The bias enters as the
// accumulators' initial value (fp32, one more term of the sum that is rounded once); the GELU epilogue stores bf(y) and bf(gelu_tanh_f(bf(y))).
#include "common.hip.h"
#include "kernels.h"

namespace ftmi {

namespace {

constexpr int W8_BM = 256, W8_BC = 128, W8_BK = 64, W8_SLOTS = 3;
constexpr int W8_SUB = 8192;            // one [64][64] bf16 sub-tile, and the byte sub-tile of W8
constexpr int W8_WOFF = 4 * W8_SUB;     // the W region of a slot, behind the four X sub-tiles
constexpr int w8_slot_bytes(bool ext) { return W8_WOFF + (ext ? 2 : 1) * W8_SUB; }

typedef __attribute__((ext_vector_type(2))) int i32x2;

struct W8Params {
    const bf16_t* X;  // [M, ldx]
    long ldx;
    const uint8_t* W8;  // [N, ldw8] bytes
    long ldw8;
    const bf16_t* bias;  // NT: [C] or null
    int M, R, C;
    const bf16_t* X2;  // [M, ldx2]
    long ldx2;
    const bf16_t* W2;  // [C, ldw2]
    long ldw2;
    int K2;
    const bf16_t* aux;  // EPI_DGELU: [M, ldaux]
    long ldaux;
    bf16_t* out;  // [M, ldo]
    long ldo;
    bf16_t* out2;  // EPI_GELU: [M, ldo2]
    long ldo2;
};

FTMI_DEVICE void w8_dma(uint32_t dst, uint32_t voff, const char* base) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(dst), "v"(voff), "s"(base) : "memory", "m0");
}

// 8 e4m3fn bytes -> 8 bf16 (an MFMA operand fragment), exact
FTMI_DEVICE s16x8 w8_frag(uint32_t lo, uint32_t hi) {
    u32x4 r;
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
    return __builtin_bit_cast(s16x8, r);
}

template <bool NN, int EPI, bool EXT>
__global__ __launch_bounds__(256, 1) void gemm_w8_kernel(W8Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TM = 4, TN = 2, SLOT = w8_slot_bytes(EXT);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, g = lane >> 5;

    const int ntm = (p.M + W8_BM - 1) / W8_BM, ntn = p.C / W8_BC;
    const int tile = xcd_remap(blockIdx.x, ntm * ntn);
    const int m0 = (tile % ntm) * W8_BM, c0 = (tile / ntm) * W8_BC;
    const int nk1 = p.R / W8_BK, S = nk1 + (EXT ? p.K2 / W8_BK : 0);

    // 64-bit tile bases; the per-lane offsets below are relative to them
    const char* xb = reinterpret_cast<const char*>(p.X + (long)m0 * p.ldx);
    const char* wb = reinterpret_cast<const char*>(p.W8) + (NN ? (long)c0 : (long)c0 * p.ldw8);
    const char* x2b = EXT ? reinterpret_cast<const char*>(p.X2 + (long)m0 * p.ldx2) : xb;
    const char* w2b = EXT ? reinterpret_cast<const char*>(p.W2 + (long)c0 * p.ldw2) : wb;

    // source offsets of this lane's pieces (see the header comment); bf16 sub-tiles: gemm_nn.hip's
    uint32_t offx[4][2], offw8[2], offx2[EXT ? 4 : 1][2], offw2[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int L = wave * 2 + i;
        if constexpr (NN) {
            const int n = L * 8 + (lane >> 3);
            offw8[i] = (uint32_t)((long)n * p.ldw8 + (((lane & 7) ^ (((n >> 1) & 3) << 1)) << 4));
        } else {
            const int r = L * 16 + (lane >> 2);
            offw8[i] = (uint32_t)((long)r * p.ldw8 + (((lane & 3) ^ ((r >> 2) & 3)) << 4));
        }
        const int row = L * 8 + (lane >> 3), slot = lane & 7;
        const int f = (((row >> 1) & 1) << 2) | ((row >> 2) & 3);
        const int cb = (slot ^ f) * 16;
        offw2[i] = EXT ? (uint32_t)((long)row * p.ldw2 * 2 + cb) : 0u;
        if constexpr (!EXT) offx2[0][i] = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long r = min(j * 64 + row, p.M - 1 - m0);  // ragged last row tile: rows past M read row M - 1 (and are never stored)
            offx[j][i] = (uint32_t)(r * p.ldx * 2 + cb);
            if constexpr (EXT) offx2[j][i] = (uint32_t)(r * p.ldx2 * 2 + cb);
        }
    }
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem);

    // the loads of stage t into ring slot `slot`: 8 of X + 2 of W8 bytes, or 8 of X2 + 4 of W2
    auto issue = [&](int t, int slot) __attribute__((always_inline)) {
        const uint32_t dst = lds0 + (uint32_t)slot * SLOT + (uint32_t)wave * 2048u;
        const bool ext = EXT && t >= nk1;
        const char* xs = ext ? x2b + (long)(t - nk1) * 128 : xb + (long)t * 128;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t o1 = offx[j][i], o2 = offx2[EXT ? j : 0][i];  // (both read as values: a select between their addresses would pin the arrays in memory)
                w8_dma(dst + j * W8_SUB + i * 1024, ext ? o2 : o1, xs);
            }
        if (ext) {
            const char* ws = w2b + (long)(t - nk1) * 128;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) w8_dma(dst + W8_WOFF + j * W8_SUB + i * 1024, offw2[i], ws + j * 64L * p.ldw2 * 2);
        } else {
            const char* ws = NN ? wb + (long)t * W8_BK * p.ldw8 : wb + (long)t * W8_BK;
#pragma unroll
            for (int i = 0; i < 2; ++i) w8_dma(dst + W8_WOFF + i * 1024, offw8[i], ws);
        }
    };

    f32x16 acc[TN][TM];
    issue(0, 0);
    if (S > 1) issue(1, 1);
    if (!NN && p.bias) {  // the bias is the sum's first term: 4 consecutive columns per register quad
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const u32x2 b = *reinterpret_cast<const u32x2*>(p.bias + c0 + wn * 64 + tn * 32 + 8 * rq + 4 * g);
                const float bv[4] = {bf2f((bf16_t)(b[0] & 0xffff)), bf2f((bf16_t)(b[0] >> 16)), bf2f((bf16_t)(b[1] & 0xffff)), bf2f((bf16_t)(b[1] >> 16))};
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[tn][tm][rq * 4 + j] = bv[j];
            }
    } else {
#pragma unroll
        for (int a = 0; a < TN; ++a)
#pragma unroll
            for (int b = 0; b < TM; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    }

    auto xfrag = [&](const char* xt, int tm, int chunk) __attribute__((always_inline)) {
        return *reinterpret_cast<const s16x8*>(xt + (tm >> 1) * W8_SUB + lds_rt_off((tm & 1) * 32 + li, chunk));
    };
    auto mfmas = [&](const s16x8 (&wf)[TN], const s16x8 (&xf)[TM]) __attribute__((always_inline)) {
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) acc[tn][tm] = mfma32(wf[tn], xf[tm], acc[tn][tm]);
    };
    // 64 reduction values of the slot at byte offset so: W8 bytes (main loop)
    auto compute_w8 = [&](int so) __attribute__((always_inline)) {
        const char* xt = smem + so + wm * 2 * W8_SUB;
        const char* wt = smem + so + W8_WOFF;
        if constexpr (NN) {
            const int u = lane >> 4, j = (lane & 15) >> 1, q = lane & 1;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                s16x8 xf[TM], wf[TN];
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) xf[tm] = xfrag(xt, tm, kk * 2 + g);
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    const int n = kk * 16 + 8 * g + j, col = wn * 64 + tn * 32 + (u & 1) * 16 + 8 * q;
                    const char* a = wt + n * 128 + (((col >> 4) ^ (((n >> 1) & 3) << 1)) << 4) + (col & 15);
                    const i32x2 b = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2*)(a));
                    wf[tn] = w8_frag((uint32_t)b[0], (uint32_t)b[1]);
                }
                mfmas(wf, xf);
            }
        } else {
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {
                u32x4 wq[TN];
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    const int r = wn * 64 + tn * 32 + li;
                    wq[tn] = *reinterpret_cast<const u32x4*>(wt + r * 64 + (((2 * pp + g) ^ ((r >> 2) & 3)) << 4));
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    s16x8 xf[TM], wf[TN];
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) xf[tm] = xfrag(xt, tm, 4 * pp + 2 * g + h);
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) wf[tn] = w8_frag(wq[tn][2 * h], wq[tn][2 * h + 1]);
                    mfmas(wf, xf);
                }
            }
        }
    };
    // ... of an extension stage: bf16 w2 [128 output columns][64], plain reads
    auto compute_ext = [&](int so) __attribute__((always_inline)) {
        const char* xt = smem + so + wm * 2 * W8_SUB;
        const char* wt = smem + so + W8_WOFF + wn * W8_SUB;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            s16x8 xf[TM], wf[TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) xf[tm] = xfrag(xt, tm, kk * 2 + g);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) wf[tn] = *reinterpret_cast<const s16x8*>(wt + lds_rt_off(tn * 32 + li, kk * 2 + g));
            mfmas(wf, xf);
        }
    };

    // epilogue geometry (gemm_nn.hip's): a wave row is 64 columns = 8 chunks of 16 bytes, a store instruction covers 8 rows
    constexpr int CPW = TN * 4, RPS = 64 / CPW, NSI = 32 / RPS;
    const int srow = lane / CPW, schunk = lane % CPW;
    u32x4 pre_in[EPI == EPI_DGELU ? TM : 1][EPI == EPI_DGELU ? NSI : 1];

    // one stage: ext: an extension stage; tail: the loop that holds the launch's last stage
    auto stage = [&](int s, int slot, bool ext, bool tail) __attribute__((always_inline)) {
        // stage s has landed (the loads of stage s + 1 may still fly: 10, or 12 when it is an extension stage), and every wave is done with the slot of stage s - 1
        if (s + 1 >= S) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        else if (EXT && s + 1 >= nk1) asm volatile("s_waitcnt vmcnt(12) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(10) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (s + 2 < S) issue(s + 2, slot == 0 ? 2 : slot - 1);
        if constexpr (EPI == EPI_DGELU) {
            if (tail && s + 1 == S) {  // the pre-activation, requested under the last stage
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int it = 0; it < NSI; ++it) {
                        const int mm = min(m0 + (wm * TM + tm) * 32 + it * RPS + srow, p.M - 1);
                        pre_in[tm][it] = *reinterpret_cast<const u32x4*>(p.aux + (long)mm * p.ldaux + c0 + wn * TN * 32 + schunk * 8);
                    }
            }
        }
        if (ext) compute_ext(slot * SLOT);
        else compute_w8(slot * SLOT);
    };
    int slot = 0;
    for (int s = 0; s < nk1; ++s) {
        stage(s, slot, false, !EXT);
        slot = slot == 2 ? 0 : slot + 1;
    }
    if constexpr (EXT) {
        // y = bf(product + bias) before the adapters' product is added: an in-register pass (the ring keeps running underneath)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tn][tm][r] = rbf(acc[tn][tm][r]);
        for (int s = nk1; s < S; ++s) {
            stage(s, slot, true, true);
            slot = slot == 2 ? 0 : slot + 1;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // the staging slots become the epilogue's scratch

    char* scr = smem + wave * (32 * CPW * 16);
    char* scr2 = smem + 4 * (32 * CPW * 16) + wave * (32 * CPW * 16);  // EPI_DGELU: the pre-activation read;  EPI_GELU: the pre-activation written
    auto scr_off = [&](int row, int chunk) { return row * (CPW * 16) + ((chunk ^ (row & (CPW - 1))) << 4); };
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        if constexpr (EPI == EPI_DGELU) {
#pragma unroll
            for (int it = 0; it < NSI; ++it) *reinterpret_cast<u32x4*>(scr2 + scr_off(it * RPS + srow, schunk)) = pre_in[tm][it];
        }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            u32x2 pk[4], pk2[EPI == EPI_GELU ? 4 : 1];
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = acc[tn][tm][rq * 4 + j];
                if constexpr (EPI == EPI_DGELU) {
                    const u32x2 zz = *reinterpret_cast<const u32x2*>(scr2 + scr_off(li, tn * 4 + rq) + 8 * g);
                    const float zv[4] = {bf2f((bf16_t)(zz[0] & 0xffff)), bf2f((bf16_t)(zz[0] >> 16)), bf2f((bf16_t)(zz[1] & 0xffff)), bf2f((bf16_t)(zz[1] >> 16))};
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = rbf(o[j]) * gelu_tanh_grad_f(zv[j]);
                }
                if constexpr (EPI == EPI_GELU) {
                    pk2[rq][0] = pack2bf(o[0], o[1]);
                    pk2[rq][1] = pack2bf(o[2], o[3]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = gelu_tanh_f(rbf(o[j]));
                }
                pk[rq][0] = pack2bf(o[0], o[1]);
                pk[rq][1] = pack2bf(o[2], o[3]);
            }
            // quads (0,1) and (2,3): after the swap lanes 0-31 hold columns [8k, 8k+8) of quad k, lanes 32-63 those of quad k+1
            auto to_scratch = [&](char* dst, const u32x2* v) __attribute__((always_inline)) {
#pragma unroll
                for (int q2 = 0; q2 < 2; ++q2) {
                    u32x4 w;
                    auto s0 = __builtin_amdgcn_permlane32_swap(v[2 * q2][0], v[2 * q2 + 1][0], false, false);
                    auto s1 = __builtin_amdgcn_permlane32_swap(v[2 * q2][1], v[2 * q2 + 1][1], false, false);
                    w[0] = s0[0]; w[1] = s1[0]; w[2] = s0[1]; w[3] = s1[1];
                    *reinterpret_cast<u32x4*>(dst + scr_off(li, tn * 4 + 2 * q2 + g)) = w;
                }
            };
            to_scratch(scr, pk);
            if constexpr (EPI == EPI_GELU) to_scratch(scr2, pk2);
        }
#pragma unroll
        for (int it = 0; it < NSI; ++it) {  // scratch -> global: 8 rows x 128 contiguous bytes per instruction, nothing past row M
            const int row = it * RPS + srow;
            const int mm = m0 + (wm * TM + tm) * 32 + row;
            const u32x4 w = *reinterpret_cast<const u32x4*>(scr + scr_off(row, schunk));
            if (mm < p.M) *reinterpret_cast<u32x4*>(p.out + (long)mm * p.ldo + c0 + wn * TN * 32 + schunk * 8) = w;
            if constexpr (EPI == EPI_GELU) {
                const u32x4 w2 = *reinterpret_cast<const u32x4*>(scr2 + scr_off(row, schunk));
                if (mm < p.M) *reinterpret_cast<u32x4*>(p.out2 + (long)mm * p.ldo2 + c0 + wn * TN * 32 + schunk * 8) = w2;
            }
        }
    }
}

template <bool NN, int EPI, bool EXT>
int launch_w8(const W8Params& p, hipStream_t st, const char* who) {
    constexpr int kSmem = W8_SLOTS * w8_slot_bytes(EXT);
    static const bool attr_ok = hipFuncSetAttribute((const void*)gemm_w8_kernel<NN, EPI, EXT>, hipFuncAttributeMaxDynamicSharedMemorySize, kSmem) == hipSuccess;
    if (!attr_ok) return set_error(FTMI_ERR_LAUNCH, NN ? "gemm_nn_w8: cannot raise the dynamic LDS limit" : "gemm_nt_w8: cannot raise the dynamic LDS limit");
    const int ntm = (p.M + W8_BM - 1) / W8_BM, ntn = p.C / W8_BC;
    hipLaunchKernelGGL((gemm_w8_kernel<NN, EPI, EXT>), dim3(ntm * ntn), dim3(256), kSmem, st, p);
    return check_launch(who);
}

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

// Every refusal of the two launchers, in gemm_nn's order; 0 when the launch may go.  Calls nothing in the runtime: the linear entries run it before their
// first launch.  The texts carry the entry's name (the literals below are spelt out per entry, set_error keeps what it is given).
int gemm_w8_refuse(const GemmW8Args& a, bool nn) {
#define W8_REFUSE(code, text) return set_error(code, nn ? "gemm_nn_w8: " text : "gemm_nt_w8: " text)
    const int R = nn ? a.N : a.K, C = nn ? a.K : a.N;  // reduction depth, output width
    const int side_epi = nn ? EPI_DGELU : EPI_GELU;
    const void* side = nn ? (const void*)a.aux : (const void*)a.out2;
    const long ldside = nn ? a.ldaux : a.ldo2;
    if (!a.X || !a.W8 || !a.out) W8_REFUSE(FTMI_ERR_INVALID, "null tensor");
    if (a.M < 1 || a.N < 1 || a.K < 1 || a.K2 < 0) W8_REFUSE(FTMI_ERR_INVALID, "empty problem or negative size");
    if (R % W8_BK != 0) return set_error(FTMI_ERR_UNSUPPORTED, nn ? "gemm_nn_w8: N (the reduction) must be a multiple of 64" : "gemm_nt_w8: K (the reduction) must be a multiple of 64");
    if (C % W8_BC != 0) return set_error(FTMI_ERR_UNSUPPORTED, nn ? "gemm_nn_w8: K (the output width) must be a multiple of 128" : "gemm_nt_w8: N (the output width) must be a multiple of 128");
    if (a.K2 % W8_BK != 0) W8_REFUSE(FTMI_ERR_UNSUPPORTED, "K2 must be a multiple of 64");
    if (a.epi != EPI_STORE && a.epi != side_epi) return set_error(FTMI_ERR_UNSUPPORTED, nn ? "gemm_nn_w8: epilogue must be 0 (store) or 3 (gelu')" : "gemm_nt_w8: epilogue must be 0 (store) or 1 (gelu)");
    if (a.epi == side_epi && !side) return set_error(FTMI_ERR_INVALID, nn ? "gemm_nn_w8: gelu' epilogue without pre-activation" : "gemm_nt_w8: gelu epilogue without out2");
    if (a.K2 > 0 && (!a.X2 || !a.W2)) W8_REFUSE(FTMI_ERR_INVALID, "K-extension without its operands");
    if (misaligned(a.X) || misaligned(a.W8) || misaligned(a.out) || misaligned(a.X2) || misaligned(a.W2) || misaligned(side) || (!nn && misaligned(a.bias)))
        W8_REFUSE(FTMI_ERR_INVALID, "tensors must keep 16-byte alignment");
    if ((a.ldx % 8) || (a.ldw8 % 16) || (a.ldo % 8) || (a.K2 > 0 && ((a.ldx2 % 8) || (a.ldw2 % 8))) || (a.epi == side_epi && (ldside % 8)))
        W8_REFUSE(FTMI_ERR_INVALID, "leading dimensions must keep 16-byte row alignment");
    if (a.ldx < R || a.ldw8 < a.K || a.ldo < C || (a.K2 > 0 && (a.ldx2 < a.K2 || a.ldw2 < a.K2)) || (a.epi == side_epi && ldside < C))
        W8_REFUSE(FTMI_ERR_INVALID, "a leading dimension is smaller than its row");
    // per-lane offsets inside a tile are 32-bit: 256 rows of x / x2, 128 (NT) or 64 (NN) rows of W8, 128 rows of w2
    if (256.0 * a.ldx * 2 >= 4294967296.0 || (nn ? 64.0 : 128.0) * a.ldw8 >= 4294967296.0 || (a.K2 > 0 && (256.0 * a.ldx2 * 2 >= 4294967296.0 || 128.0 * a.ldw2 * 2 >= 4294967296.0)))
        W8_REFUSE(FTMI_ERR_UNSUPPORTED, "a leading dimension is too large for one tile's 32-bit offsets");
    if ((long)((a.M + W8_BM - 1) / W8_BM) * (C / W8_BC) > 2147483647L) W8_REFUSE(FTMI_ERR_UNSUPPORTED, "too many tiles");
#undef W8_REFUSE
    return 0;
}

static W8Params w8_params(const GemmW8Args& a, bool nn) {
    W8Params p;
    p.X = a.X; p.ldx = a.ldx; p.W8 = a.W8; p.ldw8 = a.ldw8; p.bias = nn ? nullptr : a.bias; p.M = a.M; p.R = nn ? a.N : a.K; p.C = nn ? a.K : a.N;
    p.X2 = a.X2; p.ldx2 = a.ldx2; p.W2 = a.W2; p.ldw2 = a.ldw2; p.K2 = a.K2; p.aux = a.aux; p.ldaux = a.ldaux; p.out = a.out; p.ldo = a.ldo;
    p.out2 = a.out2; p.ldo2 = a.ldo2;
    return p;
}

int gemm_nt_w8(const GemmW8Args& a, hipStream_t st) {
    FTMI_TRY(gemm_w8_refuse(a, false));
    const W8Params p = w8_params(a, false);
    ProfScope prof(PROF_GEMM_NT, 2.0 * a.M * a.N * ((double)a.K + (double)a.K2 / 3.0), st);
    if (a.epi == EPI_GELU) return a.K2 > 0 ? launch_w8<false, EPI_GELU, true>(p, st, "gemm_nt_w8") : launch_w8<false, EPI_GELU, false>(p, st, "gemm_nt_w8");
    return a.K2 > 0 ? launch_w8<false, EPI_STORE, true>(p, st, "gemm_nt_w8") : launch_w8<false, EPI_STORE, false>(p, st, "gemm_nt_w8");
}

int gemm_nn_w8(const GemmW8Args& a, hipStream_t st) {
    FTMI_TRY(gemm_w8_refuse(a, true));
    const W8Params p = w8_params(a, true);
    ProfScope prof(PROF_GEMM_NT, 2.0 * a.M * a.K * ((double)a.N + (double)a.K2 / 3.0), st);
    if (a.epi == EPI_DGELU) return a.K2 > 0 ? launch_w8<true, EPI_DGELU, true>(p, st, "gemm_nn_w8") : launch_w8<true, EPI_DGELU, false>(p, st, "gemm_nn_w8");
    return a.K2 > 0 ? launch_w8<true, EPI_STORE, true>(p, st, "gemm_nn_w8") : launch_w8<true, EPI_STORE, false>(p, st, "gemm_nn_w8");
}

}  // namespace ftmi
