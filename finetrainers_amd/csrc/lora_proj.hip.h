// "A linear layer with its LoRA adapters" as launch descriptions, for the block orchestrators (ltx_dit / cog_dit / hy_dit / wan_dit .hip).  Everything here
// is a BUILDER: it fills and returns (or extends) an argument struct and launches nothing.  How a description is launched stays with the orchestrator --
// gemm_nt everywhere, LTX's fused down-projection + GEMM pair (lora_gemm), one batched TN launch per adapter group after the block loop (Cog, LTX).
//
//   y = x W^T + b + s (x A^T) B^T,  s = alpha / r,  W [N_out, K_in] a frozen bf16 base, A [r, K_in] and B [N_out, r] trainable fp32.  The layer may be
//   rectangular (Wan's feed-forward: K_in = D, N_out = F and the other way round); the attention projections are the square case N_out = K_in, for which
//   every builder fills exactly what it filled when it knew one width only.  `nadp` adjacent adapters on ONE input (q | k | v, k | v) ride in one launch
//   of N = nadp N_out outputs.
//
// The reference runs the adapter product in fp32 (trainer/sft_trainer/trainer.py:132-136 casts the LoRA parameters to fp32).  Here an fp32 matrix travels as two
// bf16 planes (hi, lo: kernels.h LoraSplitArgs) and a down-projected row t = s x A^T as three bf16 column planes (hi | lo | hi) per adapter: against
// an up-projection operand stored as [hi | hi | lo] columns, the K-extension of the NT GEMM then sums t_hi B_hi + t_lo B_hi + t_hi B_lo in its fp32 accumulator.
//
//   forward    XA  = s X A^T        lora_down_args over the (hi, lo) row planes of A, contracting over K_in      [M, 3 nadp r], kept for the backward
//              Y   = X W^T + XA B^T linear_args + lora_ext_fwd over B as [hi | hi | lo] columns (any epilogue of the GEMM applies to the sum)
//   backward   dXA = s dY B         lora_down_args over the (hi, lo) row planes of B^T, contracting over N_out, adapter g reading the dY columns g * xk_stride ...
//              dX  = dY W + dXA A   linear_args + lora_ext_bwd over A^T as [hi | hi | lo] columns, the nadp adapters side by side: the input gradients of
//                                   the fused projections and of their adapters are summed in ONE fp32 accumulator (the eager graph adds bf16 tensors)
//              dB += dY^T XA        lora_db_args  (XA = its hi + lo planes, folded)          [nadp N_out, r]
//              dA += dXA^T X        lora_da_args  (dXA likewise)                             [nadp r, K_in]
#pragma once
#include "common.hip.h"
#include "kernels.h"

namespace ftmi {

// out [M, N] = X W^T + bias
inline GemmNtArgs linear_args(const bf16_t* X, long ldx, int M, const bf16_t* Wm, long ldw, int N, int K, const bf16_t* bias, bf16_t* out, long ldo, int variant) {
    GemmNtArgs a;
    a.X = X; a.ldx = ldx; a.W = Wm; a.ldw = ldw; a.M = M; a.N = N; a.K = K; a.bias = bias; a.out = out; a.ldo = ldo; a.variant = variant;
    return a;
}

// out [M, 3 nadp r] = the (hi | lo | hi) planes of s * X . Af^T for `nadp` fp32 matrices Af [r, K] given as (hi, lo) row planes sp [nadp 2r, K] (the skinny split
// kernel: variant 8); K is what the product contracts over: K_in for XA (Af = A), N_out for dXA (Af = B^T).  xk_stride > 0: adapter g reads the X columns
// g * xk_stride ... (dXA of a fused projection); 0: all adapters share the input.
inline GemmNtArgs lora_down_args(const bf16_t* X, long ldx, int M, const bf16_t* sp, int nadp, int K, int r, float s, bf16_t* out, long xk_stride = 0) {
    GemmNtArgs a;
    a.X = X; a.ldx = ldx; a.W = sp; a.ldw = K; a.M = M; a.N = 2 * nadp * r; a.K = K; a.alpha = s; a.split_r = r;
    if (xk_stride > 0) { a.xk_grp_n = 2 * r; a.xk_grp_stride = xk_stride; }
    a.out = out; a.ldo = 3L * nadp * r; a.variant = 8;
    return a;
}

// + XA B^T on a forward projection `a` of a.N = nadp N_out outputs: xa [M, 3 nadp r], b_ext [nadp N_out, 3r]; adapter g adds to the output columns
// g N_out ... from its own slice of xa
inline void lora_ext_fwd(GemmNtArgs& a, const bf16_t* xa, int nadp, int r, const bf16_t* b_ext) {
    a.X2 = xa; a.ldx2 = 3L * nadp * r; a.W2 = b_ext; a.ldw2 = 3 * r; a.K2 = 3 * r;
    if (nadp > 1) { a.x2_grp_n = a.N / nadp; a.x2_grp_stride = 3 * r; }
}

// + dXA A on an input-gradient projection `a` of a.N = K_in outputs: dxa [M, 3 nadp r], at_ext [K_in, ld_at_ext] holding the adapters' A^T column groups side by side
inline void lora_ext_bwd(GemmNtArgs& a, const bf16_t* dxa, int nadp, int r, const bf16_t* at_ext, long ld_at_ext) {
    a.X2 = dxa; a.ldx2 = 3L * nadp * r; a.W2 = at_ext; a.ldw2 = ld_at_ext; a.K2 = 3 * nadp * r;
}

// dB [nadp N_out, r] += dY^T XA over M rows
inline GemmTnArgs lora_db_args(const bf16_t* dY, long lddy, const bf16_t* xa, int nadp, int r, int N_out, float* C, int M) {
    GemmTnArgs t;
    t.U = dY; t.ldu = lddy; t.V = xa; t.ldv = 3L * nadp * r; t.v_fold = r; t.C = C; t.ldc = r; t.M = M; t.P = nadp * N_out; t.Q = r;
    if (nadp > 1) { t.v_grp_p = N_out; t.v_grp_stride = 3 * r; }
    return t;
}

// dA [nadp r, K_in] += dXA^T X over M rows
inline GemmTnArgs lora_da_args(const bf16_t* dxa, int nadp, int r, const bf16_t* X, long ldx, int K_in, float* C, int M) {
    GemmTnArgs t;
    t.U = dxa; t.ldu = 3L * nadp * r; t.u_fold = r; t.V = X; t.ldv = ldx; t.C = C; t.ldc = K_in; t.M = M; t.P = nadp * r; t.Q = K_in;
    if (nadp > 1) { t.u_grp_p = r; t.u_grp_stride = 3 * r; }
    return t;
}

// the same weight-gradient product for `batch` blocks in one launch: element strides between consecutive blocks (0 = shared operand)
inline void tn_batch(GemmTnArgs& t, int batch, long u_bstride, long v_bstride, long c_bstride) {
    t.batch = batch; t.u_bstride = u_bstride; t.v_bstride = v_bstride; t.c_bstride = c_bstride;
}

// attention strides of token rows [B rows_per_batch, ld] whose heads are head_dim adjacent columns
inline void tok_strides(long& sb, long& sh, long& ss, long rows_per_batch, long ld, int head_dim) {
    sb = rows_per_batch * ld;
    sh = head_dim;
    ss = ld;
}

}  // namespace ftmi
