// NN GEMM: the input gradient of a linear layer against the weight AS THE FORWARD READS IT -- no transposed twin.
//
//   out[M, K] = epi( bf(dY[M, N] . W[N, K])  (+ X2[M, K2] . W2[K, K2]^T  when K2 > 0) )
//
// dY [M, lddy] and W [N, ldw] are row-major bf16; the reduction index n is the COLUMN of dY and the ROW of W, so W is the operand no NT kernel can read.
// X2 / W2 are the LoRA K-extension in the NT operand layout lora_ext_bwd produces (dxa [M, 3 n r], at_ext [K, ld_ext]).  Rounding points are those of the NT
// launcher's contract (include/ftmi355.h, ftmi_gemm_nt_ex): y = bf(dY W); extension: y = bf(y) + x2 w2^T; epilogue 0: out = bf(y); 3: out = bf(bf(y) gelu'(aux)).
// Reference site: autograd's grad_input of F.linear / peft lora.Linear (grad_output @ weight), which the NT path serves through W^T copies.
//
// Tile.  One workgroup (4 waves, 2 x 2) owns 256 rows x 128 output columns and walks N in 64-deep stages; a wave owns 128 rows x 64 columns = 4 x 2 MFMA tiles
// (v_mfma_f32_32x32x16_bf16, A-slot = W fragment, B-slot = dY fragment: a lane owns output row m = lane & 31 and, per register quad, 4 consecutive columns).
//
// Staging.  A stage is six [64][64] bf16 sub-tiles of 8 KiB (48 KiB): four of dY (rows 64 j ..., the stage's 64 reduction columns) and two of W (the stage's 64
// reduction ROWS x output columns 64 j ...: the two sub-tiles of a row are the two halves of ONE 256-byte K-contiguous line of W).  Every sub-tile arrives by
// eight direct-to-LDS wave loads of 1 KiB (8 rows x 128 B), in its memory layout, through the asm form of the DMA (common.hip.h says why: hipcc would otherwise
// wait for the NEXT stage's loads in front of the first transposing read).  Three slots (144 KiB): stages t + 1 and t + 2 are in flight under stage t -- the
// W rows of a stage are 64 different lines ldw apart and need the flight time --, one counted wait and ONE barrier per stage: the barrier of
// stage t also says every wave is done with slot (t - 1) % 3, which the loads of stage t + 2 issued right behind it overwrite.
//
// Fragments.  dY: ds_read_b128 of row (lane & 31), chunk 2 kk + (lane >> 5).  W: ds_read_b64_tr_b16 (lds_tr_frag): the fragment's non-reduction index is the
// sub-tile COLUMN, its 8 reduction values are LDS rows 16 kk + 8 (lane >> 5) + {0..7} -- the same n the dY chunk holds.  Swizzle: lds_rt_off for every sub-tile,
// applied to the per-lane SOURCE address of the DMA (its LDS destination is wave-linear: 16 bytes per lane, so the writes themselves are conflict-free whatever
// the swizzle).  Row r keeps chunk c in slot c ^ f(r), f a bit permutation of (r >> 1) & 7 with bit 2 = (r >> 1) & 1.  A b128 read takes 16 lanes = 16 rows at one
// chunk: the rows' f values differ in (r >> 1) & 7 and alternate row parity (128 B apart), so the 16 pieces cover the 256-byte bank row exactly once per two
// rows.  A transposing read (lds_tr_frag): inside a 16-lane group lane 4 j + q addresses 8 bytes, columns 4 q .. 4 q + 3 of row 4 m + j -- 4 rows x 32 contiguous
// bytes per group; the two groups of a 32-lane half (what one pass of a 64-bit LDS read serves: 32 x 8 B = the 256-byte bank row) take columns 0-15 and 16-31
// of the SAME four rows, so a half reads 4 rows x 64 B: chunks 4 c .. 4 c + 3 of each row.  c ^ f(r) keeps an aligned group of four chunks together (bits 0-1 of f
// permute inside it, bit 2 moves it by 64 B).  Rows 4 m, 4 m + 1 have bit 2 of f clear, rows 4 m + 2, 4 m + 3 set: 64 B apart; inside each pair the row parity puts
// the two 128-byte rows in different halves of the bank row.  Four distinct 64-byte windows = all 64 banks once: no conflict.  (lanes 32-63: rows + 8, the same.)
//
// Extension stages run after the main loop on the same ring and accumulators: the X2 sub-tiles take dY's place, W2 [128 output columns][64] takes W's and is
// read with plain ds_read_b128 (its reduction index is contiguous); bf(y) in front of them is an in-register pass over the accumulators.
//
// Epilogue (the NT kernel's): each wave transposes 32-row blocks through its own LDS scratch and stores 8 rows x 128 contiguous bytes per instruction; the
// GELU' pre-activation is requested into registers behind the barrier of the LAST stage (under its MFMAs), in the same whole-line pieces.
// Registers / LDS: see DESIGN 7-Z (128 accumulators, no scratch).  Tile order: xcd_remap over (column panel, row tile) with the row tile fastest, so the
// workgroups one XCD runs at a time share one W column panel in its L2.  All tile bases are 64-bit; per-lane offsets inside a tile are 32-bit.
#include "common.hip.h"
#include "kernels.h"

namespace ftmi {

namespace {

constexpr int NN_BM = 256, NN_BC = 128, NN_BK = 64, NN_SLOTS = 3;
constexpr int NN_SUB = 8192;                                      // one [64][64] bf16 sub-tile
constexpr int NN_SLOT_BYTES = (NN_BM / 64 + NN_BC / 64) * NN_SUB;  // 48 KiB
constexpr int NN_LPW = 2 * (NN_BM / 64 + NN_BC / 64);              // 1-KiB loads per wave and stage: 12

// one 1-KiB direct-to-LDS wave load: LDS [dst, dst + 1024) <- base + voff (per lane, 16 bytes)
FTMI_DEVICE void nn_dma(uint32_t dst, uint32_t voff, const char* base) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(dst), "v"(voff), "s"(base) : "memory", "m0");
}

template <int EPI, bool EXT>
__global__ __launch_bounds__(256, 1) void gemm_nn_kernel(GemmNnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TM = 4, TN = 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, g = lane >> 5;

    const int ntm = (p.M + NN_BM - 1) / NN_BM, ntn = p.K / NN_BC;
    const int tile = xcd_remap(blockIdx.x, ntm * ntn);
    const int m0 = (tile % ntm) * NN_BM, k0 = (tile / ntm) * NN_BC;
    const int nk1 = p.N / NN_BK, S = nk1 + (EXT ? p.K2 / NN_BK : 0);

    // 64-bit tile bases; the per-lane offsets below are relative to them
    const char* dyb = reinterpret_cast<const char*>(p.dY + (long)m0 * p.lddy);
    const char* wb = reinterpret_cast<const char*>(p.W + k0);
    const char* x2b = EXT ? reinterpret_cast<const char*>(p.X2 + (long)m0 * p.ldx2) : dyb;
    const char* w2b = EXT ? reinterpret_cast<const char*>(p.W2 + (long)k0 * p.ldw2) : wb;

    // source offsets of this lane's pieces: wave-load i of a sub-tile covers its rows (2 wave + i) 8 + (lane >> 3), slot lane & 7 <- chunk slot ^ f(row)
    uint32_t offx[4][2], offw[2], offx2[EXT ? 4 : 1][2], offw2[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (wave * 2 + i) * 8 + (lane >> 3), slot = lane & 7;
        const int f = (((row >> 1) & 1) << 2) | ((row >> 2) & 3);
        const int cb = (slot ^ f) * 16;
        offw[i] = (uint32_t)((long)row * p.ldw * 2 + cb);
        offw2[i] = EXT ? (uint32_t)((long)row * p.ldw2 * 2 + cb) : 0u;
        if constexpr (!EXT) offx2[0][i] = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long r = min(j * 64 + row, p.M - 1 - m0);  // ragged last row tile: rows past M read row M - 1 (and are never stored)
            offx[j][i] = (uint32_t)(r * p.lddy * 2 + cb);
            if constexpr (EXT) offx2[j][i] = (uint32_t)(r * p.ldx2 * 2 + cb);
        }
    }
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem);

    // the 12 loads of stage t into ring slot `slot`
    auto issue = [&](int t, int slot) __attribute__((always_inline)) {
        const uint32_t dst = lds0 + (uint32_t)slot * NN_SLOT_BYTES + (uint32_t)wave * 2048u;
        const bool ext = EXT && t >= nk1;
        const char* xs = ext ? x2b + (long)(t - nk1) * 128 : dyb + (long)t * 128;
        const char* ws = ext ? w2b + (long)(t - nk1) * 128 : wb + (long)t * NN_BK * p.ldw * 2;
        const long wstep = ext ? 64L * p.ldw2 * 2 : 128L;  // second W sub-tile: output columns 64 ... (W: the line's second half;  W2: its rows 64 ...)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t o1 = offx[j][i], o2 = offx2[EXT ? j : 0][i];  // (both read as values: a select between their addresses would pin the arrays in memory)
                nn_dma(dst + j * NN_SUB + i * 1024, ext ? o2 : o1, xs);
            }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t o1 = offw[i], o2 = offw2[i];
                nn_dma(dst + (4 + j) * NN_SUB + i * 1024, ext ? o2 : o1, ws + j * wstep);
            }
    };

    f32x16 acc[TN][TM];
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // 64 reduction values of the slot at byte offset so.  tr: the W sub-tile holds reduction ROWS (main loop); else output-column rows (extension)
    auto compute = [&](int so, bool tr) __attribute__((always_inline)) {
        const char* xt = smem + so + wm * 2 * NN_SUB;
        const char* wt = smem + so + (4 + wn) * NN_SUB;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            s16x8 xf[TM], wf[TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) xf[tm] = *reinterpret_cast<const s16x8*>(xt + (tm >> 1) * NN_SUB + lds_rt_off((tm & 1) * 32 + li, kk * 2 + g));
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                if (tr) wf[tn] = lds_tr_frag(wt, tn * 32, kk * 16 + 8 * g, kk * 16 + 8 * g + 4, lane);
                else wf[tn] = *reinterpret_cast<const s16x8*>(wt + lds_rt_off(tn * 32 + li, kk * 2 + g));
            }
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) acc[tn][tm] = mfma32(wf[tn], xf[tm], acc[tn][tm]);
        }
    };

    // epilogue geometry (see the header comment): a wave row is 64 columns = 8 chunks of 16 bytes, a store instruction covers 8 rows
    constexpr int CPW = TN * 4, RPS = 64 / CPW, NSI = 32 / RPS;
    const int srow = lane / CPW, schunk = lane % CPW;
    u32x4 pre_in[EPI == EPI_DGELU ? TM : 1][EPI == EPI_DGELU ? NSI : 1];

    // one stage: tr as in compute(); tail: the loop that holds the launch's last stage (the main loop without an extension, else the extension's)
    auto stage = [&](int s, int slot, bool tr, bool tail) __attribute__((always_inline)) {
        // stage s has landed (the NN_LPW loads of stage s + 1 may still fly), and every wave is done with the slot of stage s - 1
        if (s + 1 < S) asm volatile("s_waitcnt vmcnt(12) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        static_assert(NN_LPW == 12, "the counted wait above is written for 12 loads per wave and stage");
        if (s + 2 < S) issue(s + 2, slot == 0 ? 2 : slot - 1);
        if constexpr (EPI == EPI_DGELU) {
            if (tail && s + 1 == S) {  // the pre-activation, requested under the last stage
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int it = 0; it < NSI; ++it) {
                        const int mm = min(m0 + (wm * TM + tm) * 32 + it * RPS + srow, p.M - 1);
                        pre_in[tm][it] = *reinterpret_cast<const u32x4*>(p.aux + (long)mm * p.ldaux + k0 + wn * TN * 32 + schunk * 8);
                    }
            }
        }
        compute(slot * NN_SLOT_BYTES, tr);
    };
    issue(0, 0);
    if (S > 1) issue(1, 1);
    int slot = 0;
    for (int s = 0; s < nk1; ++s) {
        stage(s, slot, true, !EXT);
        slot = slot == 2 ? 0 : slot + 1;
    }
    if constexpr (EXT) {
        // y = bf(dY W) before the adapters' product is added: an in-register pass (the ring keeps running underneath)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tn][tm][r] = rbf(acc[tn][tm][r]);
        for (int s = nk1; s < S; ++s) {
            stage(s, slot, false, true);
            slot = slot == 2 ? 0 : slot + 1;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // the staging slots become the epilogue's scratch

    char* scr = smem + wave * (32 * CPW * 16);
    char* scr_in = smem + 4 * (32 * CPW * 16) + wave * (32 * CPW * 16);
    auto scr_off = [&](int row, int chunk) { return row * (CPW * 16) + ((chunk ^ (row & (CPW - 1))) << 4); };
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        if constexpr (EPI == EPI_DGELU) {
#pragma unroll
            for (int it = 0; it < NSI; ++it) *reinterpret_cast<u32x4*>(scr_in + scr_off(it * RPS + srow, schunk)) = pre_in[tm][it];
        }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            u32x2 pk[4];
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = acc[tn][tm][rq * 4 + j];
                if constexpr (EPI == EPI_DGELU) {
                    const u32x2 zz = *reinterpret_cast<const u32x2*>(scr_in + scr_off(li, tn * 4 + rq) + 8 * g);
                    const float zv[4] = {bf2f((bf16_t)(zz[0] & 0xffff)), bf2f((bf16_t)(zz[0] >> 16)), bf2f((bf16_t)(zz[1] & 0xffff)), bf2f((bf16_t)(zz[1] >> 16))};
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = rbf(o[j]) * gelu_tanh_grad_f(zv[j]);
                }
                pk[rq][0] = pack2bf(o[0], o[1]);
                pk[rq][1] = pack2bf(o[2], o[3]);
            }
            // quads (0,1) and (2,3): after the swap lanes 0-31 hold columns [8k, 8k+8) of quad k, lanes 32-63 those of quad k+1
#pragma unroll
            for (int q2 = 0; q2 < 2; ++q2) {
                u32x4 w;
                auto s0 = __builtin_amdgcn_permlane32_swap(pk[2 * q2][0], pk[2 * q2 + 1][0], false, false);
                auto s1 = __builtin_amdgcn_permlane32_swap(pk[2 * q2][1], pk[2 * q2 + 1][1], false, false);
                w[0] = s0[0]; w[1] = s1[0]; w[2] = s0[1]; w[3] = s1[1];
                *reinterpret_cast<u32x4*>(scr + scr_off(li, tn * 4 + 2 * q2 + g)) = w;
            }
        }
#pragma unroll
        for (int it = 0; it < NSI; ++it) {  // scratch -> global: 8 rows x 128 contiguous bytes per instruction, nothing past row M
            const int row = it * RPS + srow;
            const u32x4 w = *reinterpret_cast<const u32x4*>(scr + scr_off(row, schunk));
            const int mm = m0 + (wm * TM + tm) * 32 + row;
            if (mm < p.M) *reinterpret_cast<u32x4*>(p.out + (long)mm * p.ldo + k0 + wn * TN * 32 + schunk * 8) = w;
        }
    }
}

template <int EPI, bool EXT>
int launch_nn(const GemmNnArgs& a, hipStream_t st) {
    constexpr int kSmem = NN_SLOTS * NN_SLOT_BYTES;
    static const bool attr_ok = hipFuncSetAttribute((const void*)gemm_nn_kernel<EPI, EXT>, hipFuncAttributeMaxDynamicSharedMemorySize, kSmem) == hipSuccess;
    if (!attr_ok) return set_error(FTMI_ERR_LAUNCH, "gemm_nn: cannot raise the dynamic LDS limit");
    const int ntm = (a.M + NN_BM - 1) / NN_BM, ntn = a.K / NN_BC;
    hipLaunchKernelGGL((gemm_nn_kernel<EPI, EXT>), dim3(ntm * ntn), dim3(256), kSmem, st, a);
    return check_launch("gemm_nn");
}

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

int gemm_nn(const GemmNnArgs& a, hipStream_t st) {
    // every refusal comes before any launch (and before any call into the runtime)
    if (!a.dY || !a.W || !a.out) return set_error(FTMI_ERR_INVALID, "gemm_nn: null tensor");
    if (a.M < 1 || a.N < 1 || a.K < 1 || a.K2 < 0) return set_error(FTMI_ERR_INVALID, "gemm_nn: empty problem or negative size");
    if (a.N % NN_BK != 0) return set_error(FTMI_ERR_UNSUPPORTED, "gemm_nn: N (the reduction) must be a multiple of 64");
    if (a.K % NN_BC != 0) return set_error(FTMI_ERR_UNSUPPORTED, "gemm_nn: K (the output width) must be a multiple of 128");
    if (a.K2 % NN_BK != 0) return set_error(FTMI_ERR_UNSUPPORTED, "gemm_nn: K2 must be a multiple of 64");
    if (a.epi != EPI_STORE && a.epi != EPI_DGELU) return set_error(FTMI_ERR_UNSUPPORTED, "gemm_nn: epilogue must be 0 (store) or 3 (gelu')");
    if (a.epi == EPI_DGELU && !a.aux) return set_error(FTMI_ERR_INVALID, "gemm_nn: gelu' epilogue without pre-activation");
    if (a.K2 > 0 && (!a.X2 || !a.W2)) return set_error(FTMI_ERR_INVALID, "gemm_nn: K-extension without its operands");
    if (misaligned(a.dY) || misaligned(a.W) || misaligned(a.out) || misaligned(a.X2) || misaligned(a.W2) || misaligned(a.aux))
        return set_error(FTMI_ERR_INVALID, "gemm_nn: tensors must keep 16-byte alignment");
    if ((a.lddy % 8) || (a.ldw % 8) || (a.ldo % 8) || (a.K2 > 0 && ((a.ldx2 % 8) || (a.ldw2 % 8))) || (a.epi == EPI_DGELU && (a.ldaux % 8)))
        return set_error(FTMI_ERR_INVALID, "gemm_nn: leading dimensions must keep 16-byte row alignment");
    if (a.lddy < a.N || a.ldw < a.K || a.ldo < a.K || (a.K2 > 0 && (a.ldx2 < a.K2 || a.ldw2 < a.K2)) || (a.epi == EPI_DGELU && a.ldaux < a.K))
        return set_error(FTMI_ERR_INVALID, "gemm_nn: a leading dimension is smaller than its row");
    // per-lane offsets inside a tile are 32-bit: 256 rows of dY / X2, 64 rows of W, 128 rows of W2
    if (256.0 * a.lddy * 2 >= 4294967296.0 || 64.0 * a.ldw * 2 >= 4294967296.0 || (a.K2 > 0 && (256.0 * a.ldx2 * 2 >= 4294967296.0 || 128.0 * a.ldw2 * 2 >= 4294967296.0)))
        return set_error(FTMI_ERR_UNSUPPORTED, "gemm_nn: a leading dimension is too large for one tile's 32-bit offsets");
    if ((long)((a.M + NN_BM - 1) / NN_BM) * (a.K / NN_BC) > 2147483647L) return set_error(FTMI_ERR_UNSUPPORTED, "gemm_nn: too many tiles");
    ProfScope prof(PROF_GEMM_NT, 2.0 * a.M * a.K * ((double)a.N + (double)a.K2 / 3.0), st);
    if (a.epi == EPI_DGELU) return a.K2 > 0 ? launch_nn<EPI_DGELU, true>(a, st) : launch_nn<EPI_DGELU, false>(a, st);
    return a.K2 > 0 ? launch_nn<EPI_STORE, true>(a, st) : launch_nn<EPI_STORE, false>(a, st);
}

}  // namespace ftmi
