/* libftmi355 -- MI355X (gfx950) native kernels for the finetrainers LTX-Video LoRA SFT step.
 *
 * C ABI: plain pointers (device memory unless stated), explicit sizes/strides, a HIP stream, caller-owned
 * workspaces.  No allocation and no ownership inside the library; every call is stream-ordered (the library
 * never synchronises the device) and re-entrant.  Return value: 0 = ok, negative = error (see FTMI_ERR_*),
 * message via ftmi_last_error().
 *
 * The reference (a-r-r-o-w/finetrainers, pure Python) has no FFI; the entry points below sit behind its two
 * plugin surfaces.  Each entry names the reference interface it replaces (paths relative to the reference
 * tree):
 *
 *   ftmi_attn_fwd / ftmi_attn_bwd ...... a provider function of finetrainers/models/attention_dispatch.py:405-447
 *                                        (contract :295-362; native provider :938-962) and its autograd backward
 *   ftmi_ltx_ff_forward / ftmi_ltx_ff_backward_range the transformer call inside LTXVideoModelSpecification.forward
 *                                        (finetrainers/models/ltx_video/base_specification.py:336-342), i.e.
 *                                        _patched_LTXVideoTransformer3D_forward (finetrainers/patches/models/
 *                                        ltx_video/patch.py:38-127) + loss.backward() through it
 *                                        (finetrainers/trainer/sft_trainer/trainer.py:481)
 *   ftmi_ltx_ff_sample (+ ftmi_ltx_cfg_euler_step, _unpack_denorm) the denoising loop of the validation pipeline, latents only
 *   ftmi_ltx_ff_forward_frames / ftmi_ltx_ff_sample_cond  the same with one timestep per latent frame / the first latent frames held (image-to-video)
 *                                        (finetrainers/models/ltx_video/base_specification.py:347-377)
 *   ftmi_ltx_noise_pack ................ normalise / noise / flow-match mix / pack / target of
 *                                        base_specification.py:295-320,343,427-459 + functional/diffusion.py:4-11
 *   ftmi_mse_loss ...................... trainer/sft_trainer/trainer.py:463-480 (+ d loss / d pred)
 *   ftmi_clip_adamw_step ............... utils/torch.py:99-161,299-374 (clip_grad_norm_) +
 *                                        optimizer.py:117-125 (torch.optim.AdamW step) over the flat LoRA buffer
 *   ftmi_lora_refresh / ftmi_lora_split  (new) bf16 (hi, lo) working copies of the fp32 LoRA matrices after a step
 *   ftmi_linear_lora_fwd / _bwd ........ peft lora.Linear.forward over a frozen nn.Linear
 *                                        (trainer/sft_trainer/trainer.py:121-136 injects them) and the autograd
 *                                        backward the reference gets from loss.backward() (trainer.py:481): dgrad to
 *                                        the input, weight gradients of A and B only (the base weight is frozen)
 */
#ifndef FTMI355_H
#define FTMI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTMI_OK 0
#define FTMI_ERR_INVALID (-1)     /* bad argument (ValueError on the Python side) */
#define FTMI_ERR_UNSUPPORTED (-2) /* shape/dtype outside what the gfx950 kernels cover (ValueError) */
#define FTMI_ERR_LAUNCH (-3)      /* HIP launch/runtime failure (RuntimeError) */

typedef void* ftmi_stream; /* hipStream_t */

int ftmi_version(void);
/* Copies the message of the most recent failing call MADE BY THE CALLING THREAD (messages live in a ring tagged with the failing thread's
 * id -- the trainer's forward and the autograd engine's backward run on different threads and cannot overwrite each other's message);
 * falls back to the newest message of any thread.  No thread-local state inside the library. */
int ftmi_last_error(char* buf, size_t len);

/* In-stream HIP-event profiler used by bench.py for its live roofline figures: while enabled, every stride-th launch of a
 * kernel class is bracketed by two events on the launch stream (stride 1 = every launch; bracketing all ~1500 launches
 * of a step costs ~8 % of the step, sampling keeps the measurement inside the timed region at <1 %).  Classes: 0 gemm_nt
 * (the tiled kernel), 1 gemm_tn, 2 attention forward, 3 attention backward (dQ [+ delta] + dK/dV), 4 the skinny (N <= 256) LoRA
 * down-projection GEMM.  ftmi_prof_summary waits for the recorded
 * events and returns, for one class, the summed device time / count / algorithmic FLOPs of the SAMPLED launches and the
 * count / FLOPs of ALL launches seen (reset != 0 clears the class). */
int ftmi_prof_enable(int stride);
int ftmi_prof_summary(int kernel_class, double* sampled_ms, long* sampled_launches, double* sampled_flops, long* all_launches,
                      double* all_flops, int reset);

/* ------------------------------------------------------------------------------------------------------------
 * Attention provider level.  q,k,v,out,dout,dq,dk,dv: bf16, head_dim desc.d = 64 (LTX-Video, CogVideoX) or 128 (Wan, HunyuanVideo)
 * contiguous; element (b,h,s,:) lives at
 * base + b*stride[0] + h*stride[1] + s*stride[2] (strides in elements).  lse: fp32 [B,H,Sq] (log2 domain,
 * written by fwd, read by bwd).  key_bias: optional fp32 additive bias per (batch, head, key) (an attn_mask that broadcasts over
 * queries; desc.bias_strides = {Sk, 0} for the usual [B,Sk] mask shared by the heads), NULL for none.  A bias of -inf removes the key
 * (softmax weight exactly 0); a row whose keys ALL carry -inf has no softmax: its out row is NaN (0 / 0) and its lse -inf -- the provider
 * never sends one (the text mask keeps at least one token).  Non-causal, no dropout.
 * Refused with FTMI_ERR_INVALID before anything is launched: B, H, Sq or Sk <= 0 ("empty problem"); a null tensor; for every bf16 tensor of the call
 * (fwd: q, k, v, out; bwd also dout, dq, dk, dv -- at head_dim 64 and 128 alike) a base pointer that is not 16-byte aligned or a batch, head or token
 * stride that is not a multiple of 8 elements (the kernels move rows in 16-byte pieces; the message names the tensor).  The key bias is read one fp32
 * at a time: any strides, 4-byte alignment.  FTMI_ERR_UNSUPPORTED: desc.d other than 64 or 128.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int B, H, Sq, Sk, d;
    long q_strides[3], k_strides[3], v_strides[3], o_strides[3];
    long do_strides[3], dq_strides[3], dk_strides[3], dv_strides[3]; /* backward only */
    long bias_strides[2]; /* key_bias element (b,h,j) at key_bias[b*bias_strides[0] + h*bias_strides[1] + j]; {Sk, 0} = one row per sample */
    float scale;
} ftmi_attn_desc;

int ftmi_attn_fwd(const ftmi_attn_desc* desc, const void* q, const void* k, const void* v, void* out, float* lse,
                  const float* key_bias, ftmi_stream stream);
/* delta_ws: fp32 [B,H,Sq] scratch (rowsum(dO * O), written by the dQ kernel, read by the dK/dV kernel) */
int ftmi_attn_bwd(const ftmi_attn_desc* desc, const void* q, const void* k, const void* v, const void* out,
                  const float* lse, const void* dout, void* dq, void* dk, void* dv, float* delta_ws,
                  const float* key_bias, ftmi_stream stream);

/* Second context of a cross-attention with two key/value sets (Wan image-to-video: the CLIP image tokens next to the text tokens; two independent
 * softmaxes whose bf16 outputs are summed).  desc.d = 128, 1 <= desc.Sk <= 320, no key bias.  Run AFTER the first context's ftmi_attn_fwd / ftmi_attn_bwd:
 *   fwd: out = bf16(float(out_first) + float(bf16(softmax(q k^T scale) v))), lse [B,H,Sq] of THIS context written; out_first has desc.o_strides
 *   dq:  dq  = bf16(float(dq_first)  + float(bf16(dq of this context))); reads lse and dout; dq_first has desc.dq_strides and may be dq itself
 * rowsum(dO * O) of this context is formed inside the dq kernel (no output of this context alone is kept).  There is no dK / dV: the only caller's image
 * keys and values are frozen.  Keys past Sk are never read.
 * Refused before anything is launched: desc.d != 128 and desc.Sk > 320 (FTMI_ERR_UNSUPPORTED); Sk <= 0, H <= 0, negative B or Sq, a null tensor, and -- as
 * for ftmi_attn_fwd / ftmi_attn_bwd -- a base pointer off 16 bytes or a batch / head / token stride that is no multiple of 8 elements, for q, k, v and for
 * out_first / out (fwd), dout / dq_first / dq (dq) (FTMI_ERR_INVALID).  B == 0 or Sq == 0 returns 0 without a launch. */
int ftmi_attn_ctx2_fwd(const ftmi_attn_desc* desc, const void* q, const void* k, const void* v, const void* out_first, void* out, float* lse,
                       ftmi_stream stream);
int ftmi_attn_ctx2_dq(const ftmi_attn_desc* desc, const void* q, const void* k, const void* v, const float* lse, const void* dout, const void* dq_first,
                      void* dq, ftmi_stream stream);
/* The WIDE pair: the same contract, arguments, alignment rules and error codes for 1 <= desc.Sk <= 640 (two images in the second context: the Wan first/last-frame
 * model, 2 x 257 = 514 keys); desc.Sk > 640 is FTMI_ERR_UNSUPPORTED.  The arithmetic is the narrow pair's in the same order (64-key steps, the same online-softmax
 * updates and rounding points); what differs is the staging: two LDS slots, the next key tile on its way while the current one is multiplied, one barrier per tile,
 * in the dq kernel across its two walks.  For every Sk <= 320 the results are the narrow pair's bit for bit. */
int ftmi_attn_ctx2w_fwd(const ftmi_attn_desc* desc, const void* q, const void* k, const void* v, const void* out_first, void* out, float* lse,
                        ftmi_stream stream);
int ftmi_attn_ctx2w_dq(const ftmi_attn_desc* desc, const void* q, const void* k, const void* v, const float* lse, const void* dout, const void* dq_first,
                       void* dq, ftmi_stream stream);

/* ------------------------------------------------------------------------------------------------------------
 * Linear (+ LoRA) building block:  y = bf16( bf16(x W^T + b) + lora_scale * (x A^T) B^T ), the LoRA branch at fp32-equivalent
 * precision (peft lora.Linear with fp32 adapter weights).  a_sp [2r,K] and b_ext [N,3r] are working copies of the fp32 A [r,K] and
 * B [N,r] made by ftmi_lora_split (sp of A, ext of B); xa_out [M,3r] receives lora_scale * x A^T as bf16 planes (hi | lo | hi) and
 * is kept for the backward.  r == 0 => plain linear (a_sp, b_ext, xa_out may be NULL).
 * ------------------------------------------------------------------------------------------------------------ */
int ftmi_linear_lora_fwd(int M, int K, int N, int r, float lora_scale, const void* x, const void* w, const void* bias,
                         const void* a_sp, const void* b_ext, void* y, void* xa_out, int variant, ftmi_stream stream);

/* Backward of the above.  dy [M,N] bf16; xa [M,3r] = the forward's xa_out; w_t [K,N] = W^T (bf16, made once with
 * ftmi_transpose_bf16); bt_sp [2r,N] = t_sp of B, at_ext [K,3r] = t_ext of A (ftmi_lora_split).
 *   dxa_ws [M,3r] bf16 scratch <- lora_scale * dy B as planes (hi | lo | hi)
 *   dx [M,K] bf16            <- bf16(bf16(dy W) + dxa A)            (may be NULL: input needs no gradient)
 *   grad_a [r,K] fp32        += dxa^T x       grad_b [N,r] fp32 += dy^T xa      (accumulated, like .grad)
 * r == 0 => dx only. */
int ftmi_linear_lora_bwd(int M, int K, int N, int r, float lora_scale, const void* x, const void* dy, const void* xa,
                         const void* w_t, const void* bt_sp, const void* at_ext, void* dxa_ws, void* dx, float* grad_a,
                         float* grad_b, int variant, ftmi_stream stream);

/* Generic building blocks (exposed for tests / incremental adoption) */
/* out[M,N] = bf16(alpha * x[M,K] w[N,K]^T + bias) ; epilogue: 0 store, 1 gelu-tanh (out2 <- pre-activation),
 * 2 out = resid + (gate ? gate[b] * y : y), 3 out = y * gelu'(aux).  out2, resid and aux are [M, N] views with row stride ld_side (0: out's ldo).
 * variant: 8 = automatic kernel / tile choice (use this); 60 = the persistent 256 x 256 stream-K kernel (FTMI_ERR_UNSUPPORTED where it does
 * not apply), 61 = automatic choice among the one-tile-per-workgroup kernels only;
 * other ids pin one kernel (bit-identical A/B partners, see gemm.hip) */
int ftmi_gemm_nt(int M, int N, int K, const void* x, long ldx, const void* w, long ldw, const void* bias, float alpha,
                 void* out, long ldo, int epilogue, void* out2, const void* resid, const void* gate, int rows_per_batch,
                 const void* aux, long ld_side, int variant, ftmi_stream stream);
/* Which kernel variant 8 takes for a plain launch of this shape (K2 = depth of a fused LoRA K-extension or 0; epilogue as above), as a pure host function
 * (no device, no launch): 80 / 86 / 87 = the 16 x 16 x 32 pipeline with 256- / 192- / 224-row tiles (1386 = 192-row tiles with the W operand on a three-slot direct-to-LDS ring: the default of the 192-row launches; 2286 = 192-row tiles with the register-staged operand prefetch, FTMI_NT16_W3=0), 42 = 192 x 128 tiles (two workgroups per CU), 47 = 256 x 256
 * (8 waves), 44 = 128 x 128, 2 = a skinny kernel (N <= 256, plain store, no extension, M >= 512: the LDS-ring kernel when K % 256 == 0, else the direct-gather one), 1 = the 128 x 64 kernel of N % 128 != 0,
 * 0 = not a tiled launch (N % 64 or K % 64).  It is the launcher's own routing function applied to the plain launch (ftmi_gemm_nt_route below, for any launch): with an
 * FTMI_* switch set it reports what the launcher then does.  Host tests pin the choice to DESIGN.md. */
int ftmi_gemm_nt_plan(int M, int N, int K, int K2, int epilogue);
/* ---- in-library gradient exchange (replaces what replicate(model, bucket_cap_mb=100) does for the LoRA gradients: finetrainers/parallel/ptd.py:462-463) ----
 * One process per GPU; the collectives are RCCL's (xGMI inside a node), looked up with dlopen at the first call -- libftmi355.so has no link-time dependency on
 * librccl and these entry points return FTMI_ERR_UNSUPPORTED where it cannot be found.
 *   ftmi_allreduce_unique_id : rank 0 obtains the 128-byte rendezvous id; the host side hands the bytes to every rank (any channel: torch.distributed's store,
 *                              a file, MPI).
 *   ftmi_allreduce_init      : COLLECTIVE -- every rank calls it with the same id, its rank and the world size; creates the communicator, the library's
 *                              communication stream and its events.  The handle is owned by the caller (ftmi_allreduce_destroy).
 *   ftmi_allreduce_bucket    : all-reduce (mean if average != 0, else sum) of count fp32 values IN PLACE, ordered after everything already queued on
 *                              compute_stream (event hand-over, no host sync), running on the communication stream: the caller goes on queueing the
 *                              backward of the earlier blocks while the bucket is on the wire.  Every rank must issue the same buckets in the same order
 *                              (the block-range schedule of ftmi_ltx_ff_backward_range is a function of L alone).
 *   ftmi_allreduce_wait      : compute_stream waits (device side) for every bucket issued so far -- call before clip + AdamW.
 * Thread-safe per handle (a mutex); no thread-local state. */
typedef void* ftmi_exchange;
int ftmi_allreduce_unique_id(void* id128);
int ftmi_allreduce_init(const void* id128, int rank, int world, ftmi_exchange* out);
int ftmi_allreduce_bucket(ftmi_exchange ex, float* grad, size_t count, int average, ftmi_stream compute_stream);
int ftmi_allreduce_wait(ftmi_exchange ex, ftmi_stream compute_stream);
long ftmi_allreduce_buckets_issued(ftmi_exchange ex);
int ftmi_allreduce_version(void); /* RCCL's version code, -1 if librccl could not be loaded */
int ftmi_allreduce_destroy(ftmi_exchange ex);

/* The FTMI_* tuning switches that select between bit-identical kernels (FTMI_ATTN_PL, FTMI_ATTN_FEWKEYS, FTMI_SKINNY4) are read from the environment ONCE,
 * at the first launch that consults them -- the launch path never calls getenv.  A process that wants to compare kernels (the bit-identity tests do) changes
 * the environment and calls this: every switch consulted so far is re-read.  Returns how many were. */
int ftmi_reload_switches(void);
/* FTMI_FUSE_DOWN=1 (round 6): a LoRA down-projection and the GEMM that consumes it run as ONE launch -- the down-projection's workgroups lead the grid, the GEMM's
 * tiles wait for the rows they need on per-row-tile counters two K stages before their K-extension (csrc/gemm.hip: gemm_nt16_fused_kernel; results are the bits of
 * the two separate launches).  A wait is bounded: a poll that gives up raises a device-side status word and goes on.  This returns that word (0 = every wait of
 * every fused launch so far was satisfied); it synchronises the device -- tests only. */
int ftmi_fused_status(void);
#ifdef FTMI_EXPERIMENTAL
/* Research build only (FTMI_EXPERIMENTAL=1 python -m finetrainers_amd.csrc.build): the persistent stream-K GEMM (tools/experimental/gemm_sk.hip, variant 60) --
 * parity-green and 5-25 % slower than the shipped kernels on the step's shapes (profiles/r03_gemm_streamk.txt); not part of the product ABI. */
/* The stream-K split of the persistent GEMM as a pure host function (no device needed; tests): the last `ntiles mod n_workgroups` tiles of
 * a launch form a cost line of (nk + owner_cost) units per tile -- nk K iterations, owner_cost = what finishing the tile (LoRA extension +
 * epilogue) costs in K-iteration units -- cut into n_workgroups shares of equal cost; a cut inside a tile charges partial_cost to the workgroup
 * after it (it stores a partial) and add_cost to the tile's owner; cuts closer than min_piece iterations to a tile edge snap to it.
 * work[w] = {t0, k0, t1, k1, kinds, n_whole, contributor_mask, 0}: the share of workgroup w starts at K iteration k0 of stream-K tile t0 and
 * ends before iteration k1 of tile t1; kinds bit 0 = it opens with a partial piece (published to its owner), bit 1 = it closes with the owner
 * piece [0, k1) of tile t1; n_whole whole tiles in between; contributor_mask bit i = workgroup w + 1 + i holds a partial of that tile. */
int ftmi_gemm_sk_plan(int ntiles, int n_workgroups, int nk, int owner_cost, int min_piece, int partial_cost, int add_cost,
                      int* work /* [n_workgroups][8] */);
/* 0 = every stream-K hand-off since the previous call completed; 1 = a bounded wait for a partial gave up (results of that launch are wrong);
 * < 0 = error.  Reads and clears the word; call it after synchronising the streams that ran stream-K launches (tests and debugging only).
 * Liveness: a workgroup takes share G - 1 - blockIdx of the stream-K work, so the partials it waits for belong to workgroups that were dispatched before
 * it and publish them as their first action -- the launch makes progress whatever else occupies the device (FTMI_SK_ORDER=0 selects the first,
 * XCD-contiguous numbering, whose launches are chained across streams instead). */
int ftmi_gemm_sk_status(void);
/* Debugging aid (FTMI_SK_TRACE=1): shader-clock stamps of the last stream-K launch, out[n_workgroups][16] (start, end of each K phase,
 * hand-off waits, segment ends; 0 = unused); returns n_workgroups, 0 if nothing was traced.  Synchronises the device. */
int ftmi_gemm_sk_trace(unsigned long long* out, int capacity);
/* The wide second-context pair with the narrow pair's single-buffered staging (two barriers per tile): the yardstick of profiles/wan_flf_ctx2.txt. */
int ftmi_attn_ctx2w1_fwd(const ftmi_attn_desc* desc, const void* q, const void* k, const void* v, const void* out_first, void* out, float* lse,
                         ftmi_stream stream);
int ftmi_attn_ctx2w1_dq(const ftmi_attn_desc* desc, const void* q, const void* k, const void* v, const float* lse, const void* dout, const void* dq_first,
                        void* dq, ftmi_stream stream);
#endif /* FTMI_EXPERIMENTAL */
/* c[P,Q] (fp32) += scale * u[M,P]^T v[M,Q] */
int ftmi_gemm_tn(int M, int P, int Q, const void* u, long ldu, const void* v, long ldv, float* c, long ldc, float scale,
                 ftmi_stream stream);
/* The two GEMMs with their FULL launch description (tests: tests/test_gpu_gemm_contract.py states the contract).  Every caller-owned field of the
 * launchers' argument blocks (csrc/kernels.h: GemmNtArgs / GemmTnArgs, same names, same meaning; a zeroed block with alpha / scale = 1 and batch = 1 is the
 * plain launch).  Checked like ftmi_gemm_nt (null tensors, epilogue range, an epilogue without its input, out2 on the residual epilogue without gate2); every
 * other refusal is the launcher's own (FTMI_ERR_UNSUPPORTED / FTMI_ERR_INVALID, nothing launched).
 *   NT  y = alpha * x w^T + bias;  with a K-extension (K2 > 0)  y = bf(y) + x2 w2^T;  then the epilogue:
 *       0 out = bf(y)    1 out2 = bf(y), out = bf(gelu_tanh(out2))    3 out = bf(bf(y) * gelu_tanh'(aux))
 *       2 t = bf(y); gate: t = bf(t * gate[b, n]); out = bf(resid + t); out2 = bf(out * gate2[b, n])       (b = m / rows_per_batch; 0 = one sample)
 *       column groups: tile column n0 reads X at column offset (n0 / xk_grp_n) * xk_grp_stride (X2: x2_grp_*), W row n lives at
 *       (n / w_grp_n) * w_grp_stride + (n % w_grp_n) * ldw (W2: w2_grp_*); split_r > 0: the (hi, lo) down-projection, see ftmi_linear_lora_fwd
 *   TN  c[b][p][q] += scale * sum_m u[b][m][col(p)] v[b][m][(p / v_grp_p) * v_grp_stride + q],  col(p) = (p / u_grp_p) * u_grp_stride + p % u_grp_p;
 *       u_fold / v_fold > 0: that operand is a (hi, lo) pair of column planes this many elements apart, both contribute */
typedef struct ftmi_gemm_nt_args {
    const void* x; long ldx;
    const void* w; long ldw;
    int M, N, K;
    int xk_grp_n; long xk_grp_stride;
    int w_grp_n; long w_grp_stride;
    int w2_grp_n; long w2_grp_stride;
    const void* x2; long ldx2;
    const void* w2; long ldw2;
    int K2;
    int x2_grp_n; long x2_grp_stride;
    const void* bias;
    float alpha;
    void* out; long ldo;
    void* out2; long ldo2;
    const void* resid; long ldr;
    const void* gate; long gate_bstride;
    int rows_per_batch;
    const void* gate2; long gate2_bstride;
    const void* aux; long ldaux;
    int epilogue;
    int variant;
    int split_r;
} ftmi_gemm_nt_args;
int ftmi_gemm_nt_ex(const ftmi_gemm_nt_args* args, ftmi_stream stream);
/* What ftmi_gemm_nt_ex would run for this launch description, as a pure host function (no device, no launch; the tensor pointers are not read): the launcher
 * itself takes its decision from the same function, FTMI_* switches included.  route[0] = the kernel family: 0 nothing to do (M or N <= 0), 1 a tiled kernel of
 * the variant table, 2 the 128 x 64 tiled kernel (N or a column group no multiple of 128), 3 the LDS-ring skinny kernel, 4 / 5 the direct-gather skinny kernel with
 * a 4- / 8-way K split, 6 / 7 the 64-row split (hi, lo) kernel with 64- / 32-deep stages, 8 stream-K and 9 the 64 x 128 skinny kernel (research builds);
 * route[1] = the variant that runs after every fall-back (family 1; 0 otherwise); route[2] x route[3] = rows x columns of the output tile of one workgroup.
 * Returns 0, or the launcher's refusal (FTMI_ERR_UNSUPPORTED / FTMI_ERR_INVALID) with route[0] = 0. */
int ftmi_gemm_nt_route(const ftmi_gemm_nt_args* args, int route[4]);
typedef struct ftmi_gemm_tn_args {
    const void* u; long ldu;
    const void* v; long ldv;
    float* c; long ldc;
    int M, P, Q;
    int v_grp_p; long v_grp_stride;
    int u_grp_p; long u_grp_stride;
    long u_fold, v_fold;
    float scale;
    int batch;
    long u_bstride, v_bstride, c_bstride;
} ftmi_gemm_tn_args;
int ftmi_gemm_tn_ex(const ftmi_gemm_tn_args* args, ftmi_stream stream);
/* fp8 weight storage of the layerwise up-casting recipe (finetrainers/trainer/sft_trainer/trainer.py:111-118: storage float8_e4m3fn, compute bf16):
 * dst (bf16) = exact up-cast of src [rows, cols] (OCP e4m3fn bytes); transpose != 0: dst is [cols, rows] = src^T (rows, cols multiples of 64) -- the layout
 * the input-gradient GEMMs read.  Called per block right before it runs; 1 byte read + 2 bytes written per weight.  rows or cols <= 0: returns 0 without a
 * launch.  FTMI_ERR_INVALID: a null or not 16-byte aligned src or dst; FTMI_ERR_UNSUPPORTED: rows * cols % 16 (plain), rows % 64 or cols % 64 (transposing). */
int ftmi_fp8_upcast(const void* src, void* dst, int rows, int cols, int transpose, ftmi_stream stream);
/* out[cols,rows] = in[rows,cols]^T (bf16); used once at load time for the dgrad copies of frozen weights */
int ftmi_transpose_bf16(const void* in, void* out, int rows, int cols, ftmi_stream stream);  /* rows or cols == 0: returns 0 without a launch; negative: FTMI_ERR_INVALID */

/* Row-wise building blocks (width D = 2048; one wavefront per token row; every op of the eager chain fused in registers with a bf16
 * round wherever the reference's eager bf16 graph materialises a tensor).
 *  norm_modulate: y = bf16(bf16(norm(x)) * onep[b]) + shift[b], norm = RMSNorm (layernorm = 0) or LayerNorm (1), no affine -- the
 *    reference's _patched_rms_norm_forward (finetrainers/patches/dependencies/diffusers/rms_norm.py:17-29) / nn.LayerNorm followed by
 *    the AdaLN modulate `* (1 + scale) + shift` of the LTX block; b = row / rows_per_batch, shift / onep rows mod_bstride apart.
 *    bwd: dx = (dres ? dres + : ) norm_bwd(x, bf16(dy * onep[b])).
 *  qknorm_rope: y = rope(bf16(rms_norm(x) * w)) -- norm_q / norm_k (affine RMSNorm over the full width) followed by apply_rotary_emb
 *    (finetrainers/patches/models/ltx_video/patch.py:23-33); cos / sin fp32 [rows_per_batch, D/2] (one value per rotated pair) or NULL
 *    for no rotation (cross-attention).  bwd returns d x.  Row strides ldx / ldy / lddy / lddx in elements. */
int ftmi_norm_modulate_fwd(const void* x, const void* shift, const void* onep, long mod_bstride, void* y, int rows, int rows_per_batch,
                           int D, float eps, int layernorm, ftmi_stream stream);
int ftmi_norm_modulate_bwd(const void* x, const void* dy, const void* onep, long mod_bstride, const void* dres, void* dx, int rows,
                           int rows_per_batch, int D, float eps, int layernorm, ftmi_stream stream);
int ftmi_qknorm_rope_fwd(const void* x, long ldx, const void* w, const float* cos_t, const float* sin_t, void* y, long ldy, int rows,
                         int rows_per_batch, int D, float eps, ftmi_stream stream);
int ftmi_qknorm_rope_bwd(const void* x, long ldx, const void* w, const float* cos_t, const float* sin_t, const void* dy, long lddy,
                         void* dx, long lddx, int rows, int rows_per_batch, int D, float eps, ftmi_stream stream);
/* The same four launches with every argument of their launchers (what the DiT pass uses between its GEMMs), so that each can be tested on its own:
 *  valid_width: the row is a narrower one zero-padded to D -- means are taken over valid_width channels and the padded channels of the LayerNorm form come out
 *    as exact zeros (0 or D: the whole row).  Set around this one launch and reset.
 *  gate2 / gate2_bstride / dx2 (norm_modulate_bwd): a second output dx2 = bf16(bf16(dx) * gate2[b]) (both or neither).
 *  w_rows > 1: row i uses weight row i % w_rows of a [w_rows, D] table.   x2 / w2 / y2 (dy2 / dx2): a second tensor set with the same strides, RoPE rows and
 *    w_rows, handled by the same launch (q and k of one projection; all or none).
 *  row_grp > 0 (qknorm_rope_bwd): row i of x / dy / dx sits at row (i / row_grp) * row_grp_span + i % row_grp of its buffer (row_grp_span >= row_grp); the
 *    RoPE row and the weight row still follow i.
 * rows = 0 is an empty launch (returns 0). */
int ftmi_norm_modulate_fwd_ex(const void* x, const void* shift, const void* onep, long mod_bstride, void* y, int rows, int rows_per_batch, int D, float eps,
                              int layernorm, int valid_width, ftmi_stream stream);
int ftmi_norm_modulate_bwd_ex(const void* x, const void* dy, const void* onep, long mod_bstride, const void* dres, void* dx, int rows, int rows_per_batch, int D,
                              float eps, int layernorm, const void* gate2, long gate2_bstride, void* dx2, int valid_width, ftmi_stream stream);
int ftmi_qknorm_rope_fwd_ex(const void* x, long ldx, const void* w, const float* cos_t, const float* sin_t, void* y, long ldy, int rows, int rows_per_batch, int D,
                            float eps, int w_rows, const void* x2, const void* w2, void* y2, int valid_width, ftmi_stream stream);
int ftmi_qknorm_rope_bwd_ex(const void* x, long ldx, const void* w, const float* cos_t, const float* sin_t, const void* dy, long lddy, void* dx, long lddx, int rows,
                            int rows_per_batch, int D, float eps, int w_rows, const void* x2, const void* w2, const void* dy2, void* dx2, int row_grp,
                            int row_grp_span, int valid_width, ftmi_stream stream);

/* ------------------------------------------------------------------------------------------------------------
 * LTX-Video DiT level
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int B, S, T;      /* batch, video tokens / sample, text tokens / sample */
    int D, H, L;      /* width (2048), heads (D/H must be 64), blocks */
    int C_in, C_out;  /* latent channels (128) */
    int D_ff, D_cap;  /* 8192, 4096 */
    int r;            /* LoRA rank: 0 or a multiple of 64 */
    float lora_scale; /* alpha / r */
    float eps_norm;   /* 1e-6 (norm1 / norm2 / norm_out) */
    float eps_qk;     /* 1e-5 (norm_q / norm_k) */
    int gemm_variant; /* 8 = automatic tile / K-loop choice (production); other ids select one fixed kernel (A/B partners, gemm.hip) */
    /* 1 = gradient checkpointing (the reference's --gradient_checkpointing, trainer/sft_trainer/trainer.py:155-157 -> utils/activation_checkpoint.py:24-49,
     * every block wrapped): the workspace holds ONE block's activations instead of L (ftmi_ltx_ff_workspace_bytes shrinks accordingly), the forward keeps only
     * the residual stream, and the backward runs every block's forward kernels again right before its gradient kernels.  Gradients are bit-identical to
     * checkpoint = 0 (deterministic kernels).  Forward and backward of one step must use the same value. */
    int checkpoint;
    /* A NARROW model embedded in this layout by zero padding (round 6: the reference's dummy fixture, tests/models/ltx_video/base_specification.py:47-58 -- 4 heads x 8,
     * one block -- through the production kernels): every weight / bias / table zero-padded to D = 2048 (head h of the narrow model occupies channels [64 h, 64 h + hd)),
     * channel counts and the LoRA rank padded to multiples of 64 (finetrainers_amd/ltx_video/padded.py builds the image).  Padded channels then carry exact zeros
     * everywhere; what the kernels must be told is over how many channels a normalisation takes its mean (d_valid) and the true head width for the softmax scale
     * 1 / sqrt(head_dim_valid).  0 = the full width (2048 / 64). */
    int d_valid, head_dim_valid;
} ftmi_ltx_config;

/* All weights bf16 unless noted.  Per-block tensors are stacked along a leading L dimension.  "*_t" are
 * transposed copies (made once at load) so that every dgrad is the same K-contiguous GEMM as the forward.
 * LoRA order inside a block: 0 attn1.to_q, 1 attn1.to_k, 2 attn1.to_v, 3 attn1.to_out.0,
 *                            4 attn2.to_q, 5 attn2.to_k, 6 attn2.to_v, 7 attn2.to_out.0 */
typedef struct {
    const void *proj_in_w, *proj_in_b;                   /* [D,C_in] [D] */
    const void *time_l1_w, *time_l1_b;                   /* [D,256] [D] */
    const void *time_l2_w, *time_l2_b;                   /* [D,D] [D] */
    const void *time_lin_w, *time_lin_b;                 /* [6D,D] [6D] */
    const void *cap_l1_w, *cap_l1_b;                     /* [D,D_cap] [D] */
    const void *cap_l2_w, *cap_l2_b;                     /* [D,D] [D] */
    const void* tables;                                  /* [L,6,D] scale_shift_table of every block */
    const void* table_out;                               /* [2,D] */
    const void *proj_out_w, *proj_out_b, *proj_out_w_t;  /* [C_out,D] [C_out] [D,C_out] */
    const void *w_qkv, *b_qkv, *w_qkv_t;                 /* [L,3D,D] [L,3D] [L,D,3D] */
    const void *norm_q, *norm_k;                         /* [L,D] */
    const void *w_o, *b_o, *w_o_t;                       /* [L,D,D] [L,D] [L,D,D] */
    const void *w_q2, *b_q2, *w_q2_t;                    /* [L,D,D] [L,D] [L,D,D] */
    const void *w_kv2, *b_kv2;                           /* [L,2D,D] [L,2D] */
    const void *norm_q2, *norm_k2;                       /* [L,D] */
    const void *w_o2, *b_o2, *w_o2_t;                    /* [L,D,D] [L,D] [L,D,D] */
    const void *w_ff1, *b_ff1, *w_ff1_t;                 /* [L,D_ff,D] [L,D_ff] [L,D,D_ff] */
    const void *w_ff2, *b_ff2, *w_ff2_t;                 /* [L,D,D_ff] [L,D] [L,D_ff,D] */
    /* bf16 working copies of the fp32 LoRA matrices, refreshed by ftmi_lora_refresh.  The reference computes the LoRA branch in
     * fp32 (trainer/sft_trainer/trainer.py:132-136); here every fp32 LoRA value v travels as two bf16 numbers hi = bf16(v),
     * lo = bf16(v - hi) (16 mantissa bits) and every product is evaluated as hi*hi + lo*hi + hi*lo on the bf16 MFMA with fp32
     * accumulation -- fp32-equivalent to ~2^-16 relative. */
    const void* lora_a_sp;       /* [L,8,2r,D]  A   as (hi, lo) row planes interleaved per 32 rows: operand of x A^T      */
    const void* lora_bt_sp;      /* [L,8,2r,D]  B^T the same way:                                  operand of dY B        */
    const void* lora_b_ext;      /* [L,8,D,3r]  [B_hi | B_hi | B_lo]:   K-extension operand of the forward projections   */
    const void* lora_at_ext;     /* [L,8,D,3r]  [A^T_hi | A^T_hi | A^T_lo]: K-extension operand of the dgrads            */
    const void* lora_at_qkv_ext; /* [L,D,9r]    the same for the fused q|k|v dgrad (adapters 0,1,2 side by side)          */
    const float *rope_cos, *rope_sin; /* fp32 [S, D/2]: one (cos, sin) per rotated pair */
} ftmi_ltx_weights;

/* What every entry that runs blocks takes: the structure above, then the feed-forward adapters.  The reference hands --target_modules to peft unchanged
 * (trainer/sft_trainer/trainer.py:121-128), and its control trainer's default (trainer/control_trainer/config.py:60) names "...|ff.net.0.proj|ff.net.2": ten
 * adapters per block at one rank r and scale s = alpha / r.
 *   ff.net.0.proj  A1 [r, D], B1 [D_ff, r]:  z = n2 W1^T + b1 + (s n2 A1^T) B1^T and g = gelu(z) in one launch (K-extension under the GELU epilogue)
 *   ff.net.2       A2 [r, D_ff], B2 [D, r]:  h_out = h2 + gate (g W2^T + b2 + (s g A2^T) B2^T)
 * All eight operand pointers NULL = the eight attention adapters alone (or none, cfg->r == 0); some of them set, or any set with cfg->r == 0, is
 * FTMI_ERR_INVALID and launches nothing (a planner returns 0). */
typedef struct {
    ftmi_ltx_weights base;
    /* bf16 (hi, lo) working copies of the fp32 matrices (ftmi_lora_refresh_rect: one launch per family over the L blocks) */
    const void* ff_a1_sp;   /* [L,2r,D]     A1 as (hi, lo) row planes:              operand of n2 A1^T       */
    const void* ff_a1t_ext; /* [L,D,3r]     [A1^T_hi | A1^T_hi | A1^T_lo]:          K-extension of dn2       */
    const void* ff_b1_ext;  /* [L,D_ff,3r]  [B1_hi | B1_hi | B1_lo]:                K-extension of z         */
    const void* ff_b1t_sp;  /* [L,2r,D_ff]  B1^T as (hi, lo) row planes:            operand of dz B1         */
    const void* ff_a2_sp;   /* [L,2r,D_ff]  A2 as (hi, lo) row planes:              operand of g A2^T        */
    const void* ff_a2t_ext; /* [L,D_ff,3r]  [A2^T_hi | A2^T_hi | A2^T_lo]:          K-extension of dz        */
    const void* ff_b2_ext;  /* [L,D,3r]     [B2_hi | B2_hi | B2_lo]:                K-extension of h_out     */
    const void* ff_b2t_sp;  /* [L,2r,D]     B2^T as (hi, lo) row planes:            operand of dO B2         */
} ftmi_ltx_ff_weights;

/* Bytes of the workspace of ftmi_ltx_ff_forward / ftmi_ltx_ff_backward_range (0: a refused pointer set).  With the feed-forward adapters a block slot
 * additionally keeps "xa_ff1" and "xa_ff2" ([B*S, 3r], the down-projected rows of the two adapters), the scratch two more [B*S, 3r] buffers. */
size_t ftmi_ltx_ff_workspace_bytes(const ftmi_ltx_config* cfg, const ftmi_ltx_ff_weights* w);
/* Byte offset of a named activation inside the workspace (for tests / debugging): global names "hs" (residual
 * stream [L+1,B*S,D]; layer selects the slice), "e", "emb", "temb", "ada", "ada_out", "kv2_all" ([B*T, L*2D] text-side k|v of
 * every block), "k2n_all" ([B*T, L, D]), "xa_kv2_all"; per-block names "n1", "qkv", "qrot", "krot", "o1", "lse1", "xa_qkv",
 * "xa_o", "h1", "q2raw", "q2n", "o2", "lse2", "xa_q2", "xa_o2", "h2", "z" and, with the feed-forward adapters only, "xa_ff1", "xa_ff2". */
int ftmi_ltx_ff_workspace_offset(const ftmi_ltx_config* cfg, const ftmi_ltx_ff_weights* w, const char* name, int layer, size_t* offset);

/* Forward of the DiT (the transformer call of LTXVideoModelSpecification.forward, models/ltx_video/base_specification.py:313-330): x_t [B,S,C_in],
 * text [B,T,D_cap], key_bias fp32 [B,T] ((1-mask) * -10000 as the reference builds it), timestep fp32 [B] (= float(long(sigma*1000)),
 * base_specification.py:320; one per sample) -> pred [B,S,C_out].  Activations needed by the backward are kept in ws. */
int ftmi_ltx_ff_forward(const ftmi_ltx_config* cfg, const ftmi_ltx_ff_weights* w, const void* x_t, const void* text, const float* key_bias,
                        const float* timestep, void* pred, void* ws, size_t ws_bytes, ftmi_stream stream);

/* Forward with ONE TIMESTEP PER LATENT FRAME -- forward only.  The image-to-video mode of the reference's validation (finetrainers/models/ltx_video/
 * base_specification.py:360-361 switches to LTXImageToVideoPipeline when a validation row has an image; its training counterpart is the first-frame branch,
 * :282-311) feeds the model timestep 0 on the conditioning frame and t on the others; the oracle takes per-token timesteps as upstream does
 * (oracle/ltx.py:450-457).  Same arguments as ftmi_ltx_ff_forward, except timesteps fp32 [B, frames] (device): the S / frames tokens of latent frame f of
 * sample b are modulated by the conditioning of timesteps[b * frames + f].  S % frames == 0 and B * frames <= 128 (8 model rows x 16 latent frames, a
 * 121-frame clip; B itself is not limited to 8 here); narrow geometries (d_valid / head_dim_valid) are refused.  With all timesteps of a sample equal the
 * result is ftmi_ltx_ff_forward's, bit for bit.
 * NO BACKWARD MAY FOLLOW: cfg->checkpoint is ignored, the workspace is the checkpoint = 1 layout (one block slot + the residual stream) with conditioning
 * tables of B * frames rows -- ftmi_ltx_ff_forward_frames_workspace_bytes(cfg, w, frames) -- and ftmi_ltx_ff_backward_range would read tables of another
 * shape. */
size_t ftmi_ltx_ff_forward_frames_workspace_bytes(const ftmi_ltx_config* cfg, const ftmi_ltx_ff_weights* w, int frames);
int ftmi_ltx_ff_forward_frames(const ftmi_ltx_config* cfg, const ftmi_ltx_ff_weights* w, const void* x_t, const void* text, const float* key_bias,
                               const float* timesteps, int frames, void* pred, void* ws, size_t ws_bytes, ftmi_stream stream);

/* Backward (loss.backward() of trainer/sft_trainer/trainer.py:481): dpred [B,S,C_out] bf16 -> LoRA gradients into fp32 grad_a [L,8,r,D], grad_b [L,8,D,r]
 * and, with the feed-forward adapters (NULL without), grad_ff [L][A1 r*D | B1 D_ff*r | A2 r*D_ff | B2 D*r]: the four feed-forward gradients of a block
 * adjacent, so those of a block range are ONE contiguous slice for the gradient exchange.
 * In pieces: blocks [l_lo, l_hi) in descending order (the tail first when l_hi == L; l_hi = L, l_lo = 0 is the whole backward).  Successive calls must tile
 * L..0 (e.g. [21,28) [14,21) [7,14) [0,7)); the state between calls lives in ws.  When a call returns (stream order) the gradients of
 * all adapters of exactly those blocks are final, so a data-parallel caller starts the all-reduce of grad_a[l_lo:l_hi] /
 * grad_b[l_lo:l_hi] / grad_ff[l_lo:l_hi] on its communication stream while the next call computes -- the bucketed, overlapped gradient exchange of the
 * reference's DDP (finetrainers/parallel/ptd.py:462-463: replicate(bucket_cap_mb=100)) without a reducer.
 * accumulate = 0: the whole gradient buffer is zeroed first (by the call with l_hi == L), i.e. ".grad was None";
 * accumulate = 1: gradients are added to the buffer's content (gradient accumulation).
 * n2 and g of the feed-forward adapters are recomputed per block (norm + modulate; ftmi_gelu_from_pre on the kept z) instead of being kept: 5.5 GB over 28
 * blocks at B*S = 5376. */
int ftmi_ltx_ff_backward_range(const ftmi_ltx_config* cfg, const ftmi_ltx_ff_weights* w, const void* text, const float* key_bias, const void* dpred,
                               float* grad_a, float* grad_b, float* grad_ff, void* ws, size_t ws_bytes, int l_hi, int l_lo, int accumulate,
                               ftmi_stream stream);

/* latents, noise [B,C,F*H*W] bf16; mean,std fp32 [C]; sigma fp32 [B]; sigma_first fp32 [B] or NULL (first-frame
 * conditioning branch: tokens < first_frame_tokens use it) -> x_t, target [B,S,C] bf16.
 * B, C or S == 0: returns 0 without a launch; a negative size is FTMI_ERR_INVALID. */
int ftmi_ltx_noise_pack(const void* latents, const void* noise, const float* mean, const float* std_, const float* sigma,
                        const float* sigma_first, int first_frame_tokens, void* x_t, void* target, int B, int C, int S,
                        ftmi_stream stream);

/* ---- latent sampling (validation): the denoising loop around the forward above.  Replaces, up to the VAE decode, what the reference's validation runs
 * per prompt: LTXPipeline.__call__ as driven by LTXVideoModelSpecification.validation (finetrainers/models/ltx_video/base_specification.py:347-377;
 * [upstream] diffusers LTXPipeline + FlowMatchEulerDiscreteScheduler.step). ---- */

/* One sampler step, one pass over memory.  pred bf16 [2B, per_sample]: rows [0, B) the unconditional, [B, 2B) the conditional prediction; guidance == 1:
 * pred is [B, per_sample] and there is no unconditional half.  x fp32 [B, per_sample]: the sampler state, updated IN PLACE.  sigma, sigma_next fp32 [B]
 * (device).  All in fp32, four roundings per element:   d = c - u;  v = fma(guidance, d, u);  dt = sigma_next - sigma;  x <- fma(dt, v, x)
 * (guidance == 1: v = c).  x_next_bf16 [2B, per_sample] (guidance == 1: [B, per_sample]) receives the round-to-nearest-even bf16 copy of the new x in
 * both halves: the next model input.  per_sample % 8 == 0; tensors 16-byte aligned. */
int ftmi_ltx_cfg_euler_step(const void* pred, float* x, const float* sigma, const float* sigma_next, float guidance, void* x_next_bf16, int B,
                            long per_sample, ftmi_stream stream);

/* The same step with a HELD PREFIX: the first `hold` elements of every sample (the conditioning frames of image-to-video sampling, [upstream, unpinned]
 * LTXImageToVideoPipeline.__call__: the scheduler steps latents[:, :, 1:] only and the conditioning frame is concatenated back) are left untouched in x --
 * pred is not read there -- and only their bf16 copy goes to x_next_bf16; the other elements take the update above.  hold % 8 == 0, 0 <= hold <= per_sample;
 * hold == 0 is ftmi_ltx_cfg_euler_step. */
int ftmi_ltx_cfg_euler_step_held(const void* pred, float* x, const float* sigma, const float* sigma_next, float guidance, void* x_next_bf16, int B,
                                 long per_sample, long hold, ftmi_stream stream);

/* The inverse of ftmi_ltx_noise_pack's normalise + pack: x fp32 [B, S, C] -> latents bf16 [B, C, S] = x * std[c] + mean[c] (mean, std fp32 [C];
 * the convention of _normalize_latents, base_specification.py:427-436, scaling factor 1).  C % 4 == 0. */
int ftmi_ltx_unpack_denorm(const float* x, const float* mean, const float* std_, void* latents, int B, int C, int S, ftmi_stream stream);

/* The whole denoising loop as ONE call with no host synchronisation.  cfg->B = number of videos; the model runs at batch 2 cfg->B (unconditional rows
 * first) or, with guidance == 1, at batch cfg->B on the conditional prompt alone (text_uncond / key_bias_uncond may then be NULL).  cfg->checkpoint is
 * ignored: nothing is kept for a backward, the workspace is the checkpoint = 1 layout (one block slot + the residual stream) at the model's batch plus
 * the sampler's own buffers -- ftmi_ltx_ff_sample_workspace_bytes(cfg, w, guidance != 1).
 *   text_cond, text_uncond bf16 [B, T, D_cap]; key_bias_* fp32 [B, T] as for ftmi_ltx_ff_forward (both NULL: no mask)
 *   x fp32 [B, S, C_in]: the initial noise in packed token order on entry, the final normalised latents on return (ftmi_ltx_unpack_denorm turns them
 *     into the VAE's input)
 *   sigmas fp32 [n_steps + 1] (device), timesteps fp32 [n_steps] (device): step i feeds the model timesteps[i] for every sample and moves x from
 *     sigmas[i] to sigmas[i + 1] with ftmi_ltx_cfg_euler_step.  The caller supplies both, so the timestep rounding convention is the caller's.
 * What depends on the prompt and the adapters only -- the caption projection and the text-side k|v of every block with its LoRA extension and norm_k2
 * -- runs once per call, not once per step; w->base.rope_cos / rope_sin are the caller's tables as for the forward.  The LoRA working copies in w are
 * used as they are (refresh them after an optimiser step; the validation pipelines of base_specification.py:347-377 run the peft model as it is);
 * cfg->r == 0 samples the base model.  The result is, bit for bit, that of a loop over ftmi_ltx_ff_forward at batch 2B and ftmi_ltx_cfg_euler_step. */
size_t ftmi_ltx_ff_sample_workspace_bytes(const ftmi_ltx_config* cfg, const ftmi_ltx_ff_weights* w, int two_pass);
int ftmi_ltx_ff_sample(const ftmi_ltx_config* cfg, const ftmi_ltx_ff_weights* w, const void* text_cond, const void* text_uncond, const float* key_bias_cond,
                       const float* key_bias_uncond, float* x, const float* sigmas, const float* timesteps, int n_steps, float guidance, void* ws,
                       size_t ws_bytes, ftmi_stream stream);

/* Conditioned (image-to-video) sampling: ftmi_ltx_ff_sample with the first cond_frames of the `frames` latent frames of every sample HELD.  Replaces the
 * denoising loop of the pipeline the reference's validation builds for a row with an image (base_specification.py:360-361); restates [upstream, unpinned]
 * LTXImageToVideoPipeline.__call__:
 *   - on entry the first cond_frames * (S / frames) tokens of every sample of x are the clean, normalised conditioning latents, the rest noise; the held
 *     tokens are never written: on return they are the input, bit for bit
 *   - the model sees timestep 0 on the held frames and timesteps[i] on the others (timestep * (1 - conditioning_mask)), through the per-frame conditioning
 *     of ftmi_ltx_ff_forward_frames
 *   - the guidance combine and the Euler update apply to the other tokens only (ftmi_ltx_cfg_euler_step_held)
 * S % frames == 0, C_in % 8 == 0, (model rows) * frames <= 128.  cond_frames == 0 computes the bits of ftmi_ltx_ff_sample.  The timestep-0 conditioning row
 * is computed once per call, the embedding MLP runs on the one live timestep per step; the result is, bit for bit, that of a loop over
 * ftmi_ltx_ff_forward_frames and ftmi_ltx_cfg_euler_step_held.  No host synchronisation.  Workspace: ftmi_ltx_ff_sample_cond_workspace_bytes. */
size_t ftmi_ltx_ff_sample_cond_workspace_bytes(const ftmi_ltx_config* cfg, const ftmi_ltx_ff_weights* w, int two_pass, int frames);
int ftmi_ltx_ff_sample_cond(const ftmi_ltx_config* cfg, const ftmi_ltx_ff_weights* w, const void* text_cond, const void* text_uncond,
                            const float* key_bias_cond, const float* key_bias_uncond, float* x, const float* sigmas, const float* timesteps, int n_steps,
                            float guidance, int frames, int cond_frames, void* ws, size_t ws_bytes, ftmi_stream stream);

/* g [rows, width] = bf16(gelu_tanh(z)) from the bf16 pre-activation z a GELU GEMM stashed (row strides ldz, ldg >= width, in elements): bit for bit the g that
 * GEMM wrote next to z (both GEMM families compute the activation from the rounded z).  Replaces nothing of the reference -- its autograd keeps the
 * activation of ff.net.0 (approximate="tanh", [upstream] diffusers FeedForward) -- it is what lets the LTX backward not keep it.  16-byte vectors where bases
 * and strides are 16-byte aligned, element by element otherwise and for the width % 8 tail.  rows <= 0 or width <= 0: returns 0 without a launch. */
int ftmi_gelu_from_pre(const void* z, long ldz, void* g, long ldg, int rows, int width, ftmi_stream stream);

/* ------------------------------------------------------------------------------------------------------------
 * CogVideoX spec level (first kernels of the next model family): the DDIM noising and the velocity -> x0 conversion of
 * CogVideoXModelSpecification.forward (finetrainers/models/cogvideox/base_specification.py:283-293 and :326-329; scheduler ops
 * add_noise / get_velocity of [upstream] CogVideoXDDIMScheduler).  latents / noise / sample / outputs: bf16 [B, per_sample];
 * sqrt_alpha, sqrt_one_minus_alpha: fp32 [B] holding the scheduler's bf16-rounded sqrt(alphas_cumprod[t]), sqrt(1 - alphas_cumprod[t]).
 *   add_noise:    x0 = bf16(latents * scaling_factor)  (the training target, may be NULL);  noisy = bf16(bf16(sa x0) + bf16(so noise))
 *   get_velocity: out = bf16(bf16(sa noise) - bf16(so sample))      (the reference calls it as get_velocity(model_out, noisy, t))
 * The loss weight 1 / (1 - alphas_cumprod[t]) (utils/diffusion.py:125-128) goes through ftmi_mse_loss's per-sample weight.
 * per_sample % 8 == 0 (FTMI_ERR_UNSUPPORTED otherwise); B <= 0 or per_sample < 0: FTMI_ERR_INVALID; per_sample == 0: returns 0 without a launch.
 * ------------------------------------------------------------------------------------------------------------ */
int ftmi_ddim_add_noise(const void* latents, const void* noise, const float* sqrt_alpha, const float* sqrt_one_minus_alpha,
                        float scaling_factor, void* x0, void* noisy, int B, long per_sample, ftmi_stream stream);
int ftmi_ddim_get_velocity(const void* sample, const void* noise, const float* sqrt_alpha, const float* sqrt_one_minus_alpha, void* out,
                           int B, long per_sample, ftmi_stream stream);

/* ---- CogVideoX DiT block, row-wise stages (call sites finetrainers/models/cogvideox/base_specification.py:296-333, arithmetic
 * [upstream] diffusers CogVideoXBlock / CogVideoXLayerNormZero / Attention(qk_norm="layer_norm"), restated in oracle/cogvideox.py).
 * Tokens are one bf16 buffer [B, rows_per_batch, D] with the text_len text tokens of a sample first (the order the joint attention
 * concatenates them in); D % 64 == 0, D <= 4096.  text_len > 0: modulation tables are [B, 2, D] (row 0 text, row 1 video);
 * text_len == 0: [B, D].  Every tensor the eager bf16 graph materialises is one bf16 rounding here.  Only x-gradients exist: with LoRA on
 * the attention projections nothing upstream of the modulation / affine parameters is trainable. */
/* y = bf(bf(LayerNorm(x; w, b, eps)) * onep) + shift        (onep = bf(1 + scale), prepared by the caller like the reference's (1 + scale)) */
int ftmi_cog_ln_mod_fwd(const void* x, const void* w, const void* b, const void* shift, const void* onep, void* y, int rows, int D,
                        int rows_per_batch, int text_len, float eps, ftmi_stream stream);
/* dx = [dres +] LayerNorm'(x)[bf(dy * onep) * w]            (dres: gradient arriving on the residual branch, may be NULL) */
int ftmi_cog_ln_mod_bwd(const void* x, const void* w, const void* onep, const void* dy, const void* dres, void* dx, int rows, int D,
                        int rows_per_batch, int text_len, float eps, ftmi_stream stream);
/* q / k LayerNorm over each head's 64 channels (w, b: [64]); x, y, dy, dx: rows of D channels, row stride ld elements.
 * rope_cos / rope_sin (fp32 [S, 64], every frequency repeated twice; NULL for the sincos-table checkpoints): rotary embedding of the rotary
 * checkpoints (CogVideoX-5b), applied after the norm to the video rows only -- token position >= text_len within its rows_per_batch-token sample --
 * as diffusers' apply_rotary_emb(use_real=True, use_real_unbind_dim=-1) does on channel pairs (2i, 2i+1). */
int ftmi_cog_head_ln_fwd(const void* x, long ld, const void* w, const void* b, void* y, int rows, int D, float eps, const float* rope_cos,
                         const float* rope_sin, int rows_per_batch, int text_len, ftmi_stream stream);
int ftmi_cog_head_ln_bwd(const void* x, long ld, const void* w, const void* dy, void* dx, int rows, int D, float eps, const float* rope_cos,
                         const float* rope_sin, int rows_per_batch, int text_len, ftmi_stream stream);
/* out = res + bf(gate * y)   (res NULL: out = bf(gate * y), which is also the y-gradient of the same op) */
int ftmi_cog_gate_residual(const void* res, const void* y, const void* gate, void* out, int rows, int D, int rows_per_batch, int text_len,
                           ftmi_stream stream);

/* The whole CogVideoX block stack as one call per direction (the LTX orchestrator's design: caller-owned workspace, every activation of the backward
 * kept, nothing recomputed unless cfg->checkpoint asks for it; the backward runs over block ranges so a data-parallel caller can all-reduce finished ranges while the rest computes).
 * Weights are stacked per kind along a leading layer axis, bf16; "_t" = transposed copies for the dgrads (made once at load time). */
typedef struct {
    int B, T, S;      /* batch, text tokens, video tokens: token buffers are [B, T + S, D], text first */
    int D, H, L;      /* width = H x 64, blocks */
    int D_ff, D_temb; /* feed-forward width, time-embedding width */
    int r;            /* LoRA rank (0: none; multiple of 64) on to_q, to_k, to_v, to_out.0 */
    float lora_scale, eps_norm, eps_qk;
    int gemm_variant; /* 8 */
    /* 1 = gradient checkpointing (the reference's --gradient_checkpointing, trainer/sft_trainer/trainer.py:155-157 -> utils/activation_checkpoint.py:24-49,
     * every block wrapped; its CogVideoX recipe sets it): the workspace holds ONE block slot instead of L (ftmi_cog_workspace_bytes shrinks accordingly), the
     * forward keeps only the inputs of blocks 1 .. L-1, and the backward runs a block's forward launches again -- up to the feed-forward's pre-activation,
     * the last thing it reads; the caller's tokens_out is not touched -- right before its gradient launches, then that block's LoRA weight gradients.
     * 0 = every activation kept.  Any other value: FTMI_ERR_INVALID.  Forward and backward of one step must use the same value. */
    int checkpoint;
} ftmi_cog_config;
typedef struct {
    const void *mod_w, *mod_b;   /* [L,2,6D,D_temb], [L,2,6D]: norm1.linear and norm2.linear of every block */
    const void *norm_w, *norm_b; /* [L,2,D]: the LayerNorm affine of norm1, norm2 */
    const void *w_qkv, *b_qkv;   /* [L,3D,D], [L,3D]: to_q | to_k | to_v */
    const void *w_o, *b_o;       /* [L,D,D], [L,D] */
    const void* qk_norm;         /* [L,4,64]: norm_q.weight, norm_q.bias, norm_k.weight, norm_k.bias */
    const void *w_ff1, *b_ff1, *w_ff2, *b_ff2;       /* [L,D_ff,D], [L,D_ff], [L,D,D_ff], [L,D] */
    const void *w_qkv_t, *w_o_t, *w_ff1_t, *w_ff2_t; /* [L,D,3D], [L,D,D], [L,D,D_ff], [L,D_ff,D] */
    /* bf16 (hi, lo) working copies of the fp32 adapters (ftmi_lora_refresh_n with 4 adapters per block), NULL when r == 0 */
    const void *lora_a_sp, *lora_bt_sp, *lora_b_ext, *lora_at_ext, *lora_at_qkv_ext; /* [L,4,2r,D] x2, [L,4,D,3r] x2, [L,D,9r] */
    const float *rope_cos, *rope_sin; /* fp32 [S,64] for the rotary checkpoints, NULL otherwise */
} ftmi_cog_weights;
size_t ftmi_cog_workspace_bytes(const ftmi_cog_config* cfg);
/* tokens_out <- blocks(tokens_in); temb_silu [B, D_temb] bf16 = silu(time embedding) */
int ftmi_cog_blocks_forward(const ftmi_cog_config* cfg, const ftmi_cog_weights* w, const void* tokens_in, const void* temb_silu, void* tokens_out,
                            void* workspace, size_t workspace_bytes, ftmi_stream stream);
/* blocks [l_lo, l_hi) of the backward, last block first; ranges in descending order share the workspace.  d_tokens_out: gradient of the stack's output
 * (read when l_hi == L).  d_tokens_in (may be NULL): gradient of the stack's input (written when l_lo == 0).  grad_a [L,4,r,D] / grad_b [L,4,D,r] fp32: the
 * range's slices are overwritten (accumulate = 0) or added to (1) and are final when the call returns (stream order). */
int ftmi_cog_blocks_backward(const ftmi_cog_config* cfg, const ftmi_cog_weights* w, const void* tokens_in, const void* d_tokens_out, void* d_tokens_in,
                             float* grad_a, float* grad_b, void* workspace, size_t workspace_bytes, int l_hi, int l_lo, int accumulate, ftmi_stream stream);

/* latents [B, F, C, H, W] -> tokens [B, F (H/p) (W/p), C p p] (the im2col of CogVideoXPatchEmbed's Conv2d(kernel = stride = p), channel order
 * (c, py, px) like the flattened conv weight), and back (the model's final un-patchify).  [upstream] CogVideoXPatchEmbed / CogVideoXTransformer3DModel.
 * FTMI_ERR_INVALID before anything is launched: a null tensor, an extent or patch <= 0, H or W that is not whole patches. */
int ftmi_cog_patchify(const void* latents, void* tokens, int B, int F, int C, int H, int W, int patch, ftmi_stream stream);
int ftmi_cog_unpatchify(const void* tokens, void* latents, int B, int F, int C, int H, int W, int patch, ftmi_stream stream);

/* Precomputed-latent path (finetrainers/trainer/sft_trainer/trainer.py:374: --enable_precomputation => compute_posterior = False):
 * moments [B, 2, per_sample] bf16 = the VAE posterior (mean | logvar) as finetrainers-precomputed-data stores it, eps [B, per_sample] bf16
 * the N(0,1) draw; out = mean + exp(0.5 * clamp(logvar, -30, 20)) * eps, one bf16 rounding per torch op of
 * models/ltx_video/base_specification.py:285-289 ([upstream] diffusers DiagonalGaussianDistribution.sample).
 * per_sample % 8 == 0; B <= 0 or per_sample <= 0: FTMI_ERR_INVALID. */
int ftmi_posterior_sample(const void* moments, const void* eps, void* out, int B, long per_sample, ftmi_stream stream);

/* loss (device fp32 scalar) = mean_b mean w_b (pred-target)^2 ; dpred = d(loss*grad_scale)/dpred (bf16), may be NULL.
 * scratch: caller-owned device memory, >= FTMI_MSE_SCRATCH_FLOATS_PER_SAMPLE * B floats (per-workgroup partial sums, added in a fixed order:
 * the loss is bitwise reproducible); the library allocates nothing on this path, so the call is legal inside a stream capture.
 * per_sample % 8 == 0; B <= 0 or per_sample <= 0: FTMI_ERR_INVALID (the mean over no element is not defined; nothing is launched or written). */
#define FTMI_MSE_SCRATCH_FLOATS_PER_SAMPLE 256
int ftmi_mse_loss(const void* pred, const void* target, const float* weight, float* loss, void* dpred, int B, long per_sample,
                  float grad_scale, float* scratch, ftmi_stream stream);

/* ---- The LTX time-embedding chain, one launcher per call (used by the contract tests only; the forward passes call the launchers directly).  All tensors bf16,
 * dense, 16-byte aligned.  A zero size returns 0 without a launch, a negative one is FTMI_ERR_INVALID.
 *   timestep_sinusoid  t fp32 [B] -> out [B, 256] = bf([cos(t f_j) | sin(t f_j)]), f_j = expf(-ln(10000) j / 128), j < 128
 *   small_linear       y [rows, N] = bf(sum_k xin[r][k] w[n][k] + bias[n]), xin = silu_in ? bf(silu(x)) : x;  x [rows, K], w [N, K], bias [N] or NULL;
 *                      rows 1..8 and K % 8 == 0 (FTMI_ERR_UNSUPPORTED otherwise)
 *   ada_prep           tables [L, 6, D], temb [B, 6, D] -> ada [L, B, 8, D]: slots 0..5 = bf(table + temb), 6 = bf(1 + slot 1), 7 = bf(1 + slot 4)
 *   ada_out_prep       table2 [2, D], emb [B, D] -> ada_out [B, 3, D]: shift = bf(table2[0] + emb), scale = bf(table2[1] + emb), bf(1 + scale) */
int ftmi_timestep_sinusoid(const float* t, void* out, int B, ftmi_stream stream);
int ftmi_small_linear(const void* x, const void* w, const void* bias, void* y, int rows, int N, int K, int silu_in, ftmi_stream stream);
int ftmi_ada_prep(const void* tables, const void* temb, void* ada, int L, int B, int D, ftmi_stream stream);
int ftmi_ada_out_prep(const void* table2, const void* emb, void* ada_out, int B, int D, ftmi_stream stream);

/* Global L2 clip (max_norm <= 0 disables) + AdamW over flat fp32 buffers; scratch: >= FTMI_CLIP_SCRATCH_FLOATS floats (device).
 * The norm is reduced in a fixed order (block partials in scratch, last block adds them): the same gradients give the same
 * bits on every call and on every rank, so data-parallel replicas keep identical clip coefficients.
 * grad_norm_out (device fp32, may be NULL) receives the pre-clip total norm.
 * The bias corrections 1 - beta^step are computed in double from the fp32 betas and rounded to fp32 once (as ftmi_adamw_bf16_step does).
 * n == 0: returns 0 without a launch, nothing is written (grad_norm_out included); n < 0: FTMI_ERR_INVALID. */
#define FTMI_CLIP_SCRATCH_FLOATS 2050
int ftmi_clip_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float max_norm, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int step, float* scratch, float* grad_norm_out,
                         ftmi_stream stream);

/* In-place global L2 clip of a flat fp32 gradient buffer: grads *= min(1, max_norm / (norm + 1e-6)) (finetrainers/utils/torch.py:99-161).
 * The reference loop clips after EVERY backward (trainer/sft_trainer/trainer.py:487-492), also on the micro-steps of a gradient-
 * accumulation window where no optimiser step follows; ftmi_clip_adamw_step covers the stepping micro-step, this call the others.
 * scratch: >= FTMI_CLIP_SCRATCH_FLOATS floats; grad_norm_out (may be NULL) receives the pre-clip norm; order-fixed reduction.
 * max_norm <= 0 disables the clip (the norm is still written); n <= 0: FTMI_ERR_INVALID. */
int ftmi_clip_grad_norm(float* grads, long n, float max_norm, float* scratch, float* grad_norm_out, ftmi_stream stream);

/* HunyuanVideo ([upstream] diffusers Attention(qk_norm = "rms_norm") + HunyuanVideoAttnProcessor2_0, restated in oracle/hunyuan.py): q / k
 * RMSNorm over each head's head_dim channels (128; weight [head_dim] bf16, eps 1e-6, the reference's patched F.rms_norm: one bf16 rounding), then -- on
 * the rows at position >= rope_from of a sample of rows_per_batch tokens (the video tokens of a joint [text | video] sequence) -- the rotary embedding
 * in its real form: rope_cos / rope_sin fp32 [rows_per_batch - rope_from, head_dim], every frequency repeated for its channel pair; NULL: none.
 * x / y / dy / dx: [rows, D] bf16 views with their own row strides (multiples of 8, at least D).  D is a multiple of head_dim (a row is whole heads).
 * Only the input gradient is produced (LoRA training). */
int ftmi_head_rms_rope_fwd(const void* x, long ld, const void* w, void* y, long ld_y, int rows, int D, int head_dim, float eps, const float* rope_cos,
                           const float* rope_sin, int rows_per_batch, int rope_from, ftmi_stream stream);
int ftmi_head_rms_rope_bwd(const void* x, long ld, const void* w, const void* dy, long ld_dy, void* dx, long ld_dx, int rows, int D, int head_dim, float eps,
                           const float* rope_cos, const float* rope_sin, int rows_per_batch, int rope_from, ftmi_stream stream);

/* HunyuanVideo single-stream block (40 of the 60 blocks of the DiT; [upstream] diffusers HunyuanVideoSingleTransformerBlock as driven by
 * finetrainers/models/hunyuan_video/base_specification.py:294-330, restated in oracle/hunyuan.py SingleStreamBlock) as ONE call per direction:
 *   tokens x [B, T + S, D] bf16 (text first), temb_silu [B, D] = silu(conditioning vector), key_bias fp32 [B, T + S] (-inf on padded text keys) or NULL,
 *   rope_cos / rope_sin fp32 [S, 128] (video rows), LoRA (fp32, rank r, scale alpha / r) on to_q / to_k / to_v.
 * Buffers are the caller's: `saved` (ftmi_hy_single_saved_bytes: what the backward reads again -- keep it from the forward to the backward of THIS block,
 * or rebuild it inside the backward by calling the forward with out = NULL, which is gradient checkpointing: utils/activation_checkpoint.py:24-49) and
 * `scratch` (ftmi_hy_single_scratch_bytes: transients, may be shared by all blocks on a stream).  The weights may be views into an arena that is
 * refilled per block (fp8 storage: ftmi_fp8_upcast).  The backward ADDS to grad_a [3, r, D] / grad_b [3, D, r] (fp32) and writes dx. */
typedef struct {
    int B, T, S;      /* batch, text tokens, video tokens */
    int D, H, mlp;    /* width = H x 128, MLP width (4 D) */
    int r;            /* LoRA rank: 0 or a multiple of 64 (smaller ranks zero-padded by the caller) */
    float lora_scale; /* alpha / (the user's) r */
    float eps;        /* 1e-6: LayerNorm and q / k RMSNorm */
    int gemm_variant; /* 8 */
} ftmi_hy_single_config;
typedef struct {
    const void *norm_lin_w, *norm_lin_b;                       /* [3D, D], [3D]   norm.linear */
    const void *proj_mlp_w, *proj_mlp_b;                       /* [mlp, D], [mlp] */
    const void *wq, *bq, *wk, *bk, *wv, *bv;                   /* [D, D], [D]     attn.to_q / to_k / to_v */
    const void *norm_q_w, *norm_k_w;                           /* [128]           attn.norm_q / norm_k */
    const void *proj_out_w, *proj_out_b;                       /* [D, D + mlp], [D] */
    const void *wq_t, *wk_t, *wv_t, *proj_mlp_w_t, *proj_out_w_t; /* transposed copies [D, D] x3, [D, mlp], [D + mlp, D]: backward only */
    const float *lora_a, *lora_b;                              /* fp32 [3, r, D], [3, D, r]; NULL when r == 0 */
    const void *ones, *zeros;                                  /* bf16 [D]: the affine-free LayerNorm's weight and bias */
} ftmi_hy_single_weights;
size_t ftmi_hy_single_saved_bytes(const ftmi_hy_single_config* cfg);
size_t ftmi_hy_single_scratch_bytes(const ftmi_hy_single_config* cfg);
/* out [B, T + S, D]; out == NULL: recomputation pass (fills `saved`, stops after the attention) */
int ftmi_hy_single_forward(const ftmi_hy_single_config* cfg, const ftmi_hy_single_weights* w, const void* x, const void* temb_silu, const float* key_bias,
                           const float* rope_cos, const float* rope_sin, void* out, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                           ftmi_stream stream);
/* ones_rows: bf16 [B, D] of 1.0 (the bf16 accumulation of the four gradients of the normalised tokens runs through the gate-residual kernel) */
int ftmi_hy_single_backward(const ftmi_hy_single_config* cfg, const ftmi_hy_single_weights* w, const void* x, const void* dout, const float* key_bias,
                            const float* rope_cos, const float* rope_sin, const void* ones_rows, void* dx, float* grad_a, float* grad_b, void* saved,
                            size_t saved_bytes, void* scratch, size_t scratch_bytes, ftmi_stream stream);

/* HunyuanVideo dual-stream block (the other 20 blocks; [upstream] diffusers HunyuanVideoTransformerBlock, oracle/hunyuan.py DualStreamBlock), ONE SAMPLE per
 * call: video x_v [S, D] and text x_t [T, D] keep their own modulation (temb_silu [1, D]), projections, q / k norms and feed-forward and meet in one joint
 * attention over [text | video] (key_bias fp32 [T + S] or NULL; rope_cos / rope_sin fp32 [S, 128] on the video rows); LoRA (adapters 0..3) on the video
 * stream's to_q / to_k / to_v / to_out.0 and, with text_adapters = 1, (adapters 4..7) on the text stream's add_q_proj / add_k_proj / add_v_proj / to_add_out:
 * lora_a / lora_b / grad_a / grad_b then hold eight matrices in that order, `saved` also keeps the text rows' down-projections (the recomputation pass
 * refills them) and `scratch` holds eight operand copies and a down-projection gradient of max(S, T) rows.  text_adapters = 0 is the layout, the launch
 * sequence and the result without the field; text_adapters = 1 with r = 0, or any other value, is FTMI_ERR_INVALID before any launch (0 bytes from the
 * two planners).
 * Buffers and gradient semantics as for the single-stream block; out_v == out_t == NULL: recomputation pass. */
typedef struct {
    int T, S;         /* text tokens, video tokens of the sample */
    int D, H, mlp;    /* width = H x 128, feed-forward width */
    int r;            /* LoRA rank: 0 or a multiple of 64 */
    float lora_scale, eps;
    int gemm_variant; /* 8 */
    int text_adapters; /* 0: adapters on the video stream only; 1: also on the text stream (needs r > 0) */
} ftmi_hy_dual_config;
typedef struct {
    const void *norm1_lin_w, *norm1_lin_b, *norm1c_lin_w, *norm1c_lin_b;              /* [6D, D], [6D]: norm1.linear, norm1_context.linear */
    const void *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo;                                /* video: attn.to_q / to_k / to_v / to_out.0 */
    const void *add_q_w, *add_q_b, *add_k_w, *add_k_b, *add_v_w, *add_v_b, *add_out_w, *add_out_b; /* text: attn.add_*_proj, attn.to_add_out */
    const void *norm_q_w, *norm_k_w, *norm_added_q_w, *norm_added_k_w;                /* [128] */
    const void *ff1_w, *ff1_b, *ff2_w, *ff2_b, *ffc1_w, *ffc1_b, *ffc2_w, *ffc2_b;    /* [mlp, D], [mlp], [D, mlp], [D]: ff, ff_context */
    const void *wq_t, *wk_t, *wv_t, *wo_t, *add_q_w_t, *add_k_w_t, *add_v_w_t, *add_out_w_t, *ff1_w_t, *ff2_w_t, *ffc1_w_t, *ffc2_w_t; /* transposed: backward only */
    const float *lora_a, *lora_b;                                                     /* fp32 [4, r, D], [4, D, r] ([8, ..] with text_adapters); NULL when r == 0 */
    const void *ones, *zeros;                                                         /* bf16 [D] */
} ftmi_hy_dual_weights;
size_t ftmi_hy_dual_saved_bytes(const ftmi_hy_dual_config* cfg);
size_t ftmi_hy_dual_scratch_bytes(const ftmi_hy_dual_config* cfg);
int ftmi_hy_dual_forward(const ftmi_hy_dual_config* cfg, const ftmi_hy_dual_weights* w, const void* x_v, const void* x_t, const void* temb_silu,
                         const float* key_bias, const float* rope_cos, const float* rope_sin, void* out_v, void* out_t, void* saved, size_t saved_bytes,
                         void* scratch, size_t scratch_bytes, ftmi_stream stream);
/* ones_row: bf16 [D] of 1.0; grad_a [4, r, D] / grad_b [4, D, r] fp32 ([8, ..] with text_adapters) are ADDED to */
int ftmi_hy_dual_backward(const ftmi_hy_dual_config* cfg, const ftmi_hy_dual_weights* w, const void* x_v, const void* x_t, const void* dout_v, const void* dout_t,
                          const float* key_bias, const float* rope_cos, const float* rope_sin, const void* ones_row, void* dx_v, void* dx_t, float* grad_a,
                          float* grad_b, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, ftmi_stream stream);

/* ---- Wan-T2V full fine-tune (BASELINE config 4; finetrainers/models/wan/base_specification.py:433-493 driving [upstream]
 * diffusers transformer_wan.py; restated in oracle/wan.py).  Every parameter trains, so the backward kernels also produce the column sums the
 * parameter gradients need; they ADD to red1 / red2 (fp32, zeroed or kept by the caller; atomics: the summation order is not fixed).
 * One argument block for the seven row-wise launchers; rows = whole samples of rows_per_batch tokens, D a multiple of 64 (<= 4096, colsum: any),
 * row strides multiples of 8.
 *   ftmi_wan_ln_fwd        y = bf(LN(float(x)) [* w + b] [* (1 + scale_b) + shift_b])     FP32LayerNorm (+ affine | + modulation), one rounding
 *   ftmi_wan_ln_bwd        y = dx = bf([dres +] bf(LN'(x)[dy * (w | 1 + scale_b)]));  red1 += sum dy (d shift | d bias), red2 += sum dy * xhat
 *                          (d scale | d weight); red_per_batch = 1 for the modulated norms ([B, D] sums)
 *   ftmi_wan_rms_rope_fwd  n = bf(x * rstd(x) * w) over the WHOLE row (qk_norm = "rms_norm_across_heads"), y = bf(n rotated by rope_cos/sin
 *                          [rows_per_batch, head_dim / 2], the complex pair (2k, 2k+1) of every head times cos_k + i sin_k); rope null: y = n
 *   ftmi_wan_rms_rope_bwd  y = dx;  red2 += sum dn * xhat (d weight)
 *   ftmi_wan_gate_res_fwd  y = bf(float(x) + float(dy) * scale_b)   ("dy" = the branch output; scale = fp32 gate [B, D], null: bf(x + dy))
 *   ftmi_wan_gate_res_bwd  x = d out, dy = the branch output of the forward: y = bf(d out * scale_b), red1 += sum d out * branch (d gate);
 *                          red1 NULL (a frozen gate): dy is not read and may be NULL
 *   ftmi_wan_colsum        red1 += sum over rows of x   (Linear bias gradients) */
typedef struct ftmi_wan_row_args {
    const void* x; long ld_x;
    const void* w; const void* b;            /* bf16 [D] */
    const float* shift; const float* scale;  /* fp32 [B, mod_bstride] */
    long mod_bstride;
    const void* dy; long ld_dy;
    const void* dres;                        /* bf16, row stride ld_y */
    void* y; long ld_y;
    float* red1; float* red2; int red_per_batch;
    const float* rope_cos; const float* rope_sin; int head_dim;
    int rows, D, rows_per_batch;
    float eps;
} ftmi_wan_row_args;
int ftmi_wan_ln_fwd(const ftmi_wan_row_args* args, ftmi_stream stream);
int ftmi_wan_ln_bwd(const ftmi_wan_row_args* args, ftmi_stream stream);
int ftmi_wan_rms_rope_fwd(const ftmi_wan_row_args* args, ftmi_stream stream);
int ftmi_wan_rms_rope_bwd(const ftmi_wan_row_args* args, ftmi_stream stream);
int ftmi_wan_gate_res_fwd(const ftmi_wan_row_args* args, ftmi_stream stream);
int ftmi_wan_gate_res_bwd(const ftmi_wan_row_args* args, ftmi_stream stream);
int ftmi_wan_colsum(const ftmi_wan_row_args* args, ftmi_stream stream);

/* One Wan-T2V DiT block (the unit FSDP-2 shards, finetrainers/parallel/ptd.py:466-499) as ONE call per direction.  params: the block's flat bf16 parameter
 * buffer in the order of finetrainers_amd/wan/block.py WanBlockLayout (ftmi_wan_block_param_elements elements: attn1 q|k|v weights, their biases, attn1
 * to_out, attn1 norm_q / norm_k, attn2 to_q, attn2 k|v weights, their biases, attn2 to_out, attn2 norm_q / norm_k, norm2, ffn.net.0.proj, ffn.net.2,
 * scale_shift_table) -- the local buffer or the all-gathered one; grads: fp32, same layout, ADDED to (every entry except scale_shift_table, whose
 * gradient the caller forms from dmod).  x [B, S, D], enc [B, T, D] bf16; mod fp32 [B, 6, D] = scale_shift_table + time projection; rope_cos / rope_sin
 * fp32 [S, 64].  `saved` (ftmi_wan_block_saved_bytes) must live from the forward to the backward of the block; `scratch` (ftmi_wan_block_scratch_bytes,
 * backward only) may be shared by all blocks of a stream.  dmod fp32 [6, B, D] is ADDED to (per-sample column sums of d shift / d scale / d gate). */
typedef struct {
    int B, S, T;      /* batch, video tokens, text tokens */
    int D, H, F;      /* width = H x 128 <= 5120, feed-forward width */
    float eps;        /* 1e-6 */
    int gemm_variant; /* 8 */
} ftmi_wan_block_config;
size_t ftmi_wan_block_saved_bytes(const ftmi_wan_block_config* cfg);
size_t ftmi_wan_block_scratch_bytes(const ftmi_wan_block_config* cfg);
size_t ftmi_wan_block_param_elements(const ftmi_wan_block_config* cfg);
int ftmi_wan_block_forward(const ftmi_wan_block_config* cfg, const void* params, const void* x, const void* enc, const float* mod, const float* rope_cos,
                           const float* rope_sin, void* out, void* saved, size_t saved_bytes, ftmi_stream stream);
int ftmi_wan_block_backward(const ftmi_wan_block_config* cfg, const void* params, float* grads, const void* x, const void* enc, const float* mod,
                            const float* rope_cos, const float* rope_sin, const void* dout, void* dx, void* denc, float* dmod, void* saved, size_t saved_bytes,
                            void* scratch, size_t scratch_bytes, ftmi_stream stream);

/* The same block for LoRA fine-tuning over a FROZEN base, text-to-video and image-to-video: ONE entry family, ftmi_wan_lora_ffn_block_*, and the same forward
 * and backward walk behind it as behind ftmi_wan_block_* (one implementation, csrc/wan_dit.hip).  The configuration is ftmi_wan_block_config plus r and
 * lora_scale (the adapters), TI (the image context) and ffn (adapters on the feed-forward projections as well).
 *
 * Attention adapters (the reference's Wan SFT recipes: --training_type lora --target_modules "blocks.*(to_q|to_k|to_v|to_out.0)"): fp32 lora_a [8, r, D] /
 * lora_b [8, D, r] sit on attn1.to_q, to_k, to_v, to_out.0, attn2.to_q, to_k, to_v, to_out.0 (in this order) and every projection computes
 * x W^T + b + lora_scale (x A^T) B^T.  params: the flat bf16 buffer as above; w_*_t: K-contiguous (transposed) twins of the seven weight matrices, backward
 * only -- [D, 3D] of attn1 q|k|v, [D, D] of attn1.to_out.0, attn2.to_q, [D, 2D] of attn2 k|v, [D, D] of attn2.to_out.0, [D, F] of ffn.net.0.proj, [F, D] of
 * ffn.net.2.  x [B, S, D], enc [B, T, D] bf16, mod fp32 [B, 6, D], rope_cos / rope_sin fp32 [S, 64] as above.
 * `saved` (ftmi_wan_lora_ffn_block_saved_bytes; smaller than the full fine-tune's by B S (3D + F) 2 bytes, larger by the down-projected rows) lives from the
 * forward to the backward of the block, or is rebuilt inside the backward by calling the forward with out = NULL (gradient checkpointing: the recomputation
 * pass refills `saved` with the identical kernel sequence, the feed-forward adapters' rows included); `scratch` (ftmi_wan_lora_ffn_block_scratch_bytes, both
 * directions) may be shared by all blocks of a stream.  With r = 0 the forward's output and the backward's dx are those of ftmi_wan_block_forward /
 * _backward, bit for bit.  The backward writes dx, writes denc unless it is NULL (frozen text embedder: that GEMM is skipped) and ADDS to grad_a [8, r, D] /
 * grad_b [8, D, r] (fp32); no base-weight, norm, bias or modulation gradient is formed.
 *
 * Image context (TI > 0; a Wan image-to-video model, Wan2.1-I2V: attn2 has added_kv_proj_dim): the cross-attention becomes
 *   o2 = bf(SDPA(q2, k_text, v_text)) + bf(SDPA(q2, k_img, v_img)),  k_img = norm_added_k(add_k_proj(enc_img)),  v_img = add_v_proj(enc_img).
 * TI is the number of image tokens (257); enc_img [B, TI, D] bf16 is the image embedder's output.  img_params: a SEPARATE flat bf16 buffer (the block's own
 * flat buffer keeps its layout): add_k_proj | add_v_proj weight [2D, D], their biases [2D], norm_added_k weight [D].  No adapter sits on them (the recipe's
 * regex does not match), so the backward adds only the image branch's dQ: no gradient to enc_img or to img_params.  `saved` grows by the projected image
 * rows [B TI, 3D], lse of the image branch and the summed attention output [B, S, D]; `scratch` does not depend on TI.  TI = 0 (text-to-video; img_params /
 * enc_img may then be NULL): none of it -- no launch, no byte.
 * A second image (TI2 > 0; the first/last-frame model, Wan2.1-FLF2V, whose image embedder carries pos_embed): its TI2 tokens follow the first image's in
 * enc_img [B, TI + TI2, D]; the image GEMM and RMSNorm run over B (TI + TI2) rows, the projected rows in `saved` grow to that count (nothing else moves) and both
 * directions call ftmi_attn_ctx2w_* with Sk = TI + TI2.  TI2 = 0: the plans, launches and bits of the single image.  TI2 needs TI > 0; each is at most 320.
 * (ftmi_wan_lora_ffn_block_config and ftmi_wan_sample_config grew by this one trailing int without a version step: ftmi_version() stays 101, and the Python
 * structures of finetrainers_amd/_lib.py are their only callers.)
 *
 * Feed-forward adapters (ffn = 1): ffn.net.0.proj (A_1 [r, D], B_1 [F, r]) and ffn.net.2 (A_2 [r, F], B_2 [D, r]) next to the eight attention projections,
 * at the same rank and scale -- what peft attaches when the reference's --target_modules (handed over unchanged: finetrainers/trainer/sft_trainer/trainer.py:121-128
 * builds LoraConfig(r, lora_alpha, target_modules) and calls transformer.add_adapter) also names "ffn.net.0.proj" and "ffn.net.2"; they are the two "ff"
 * members of the control trainer's default list (finetrainers/trainer/control_trainer/config.py:60-62
 * --target_modules "(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|ff.net.0.proj|ff.net.2)") spelled for Wan, whose feed-forward
 * module is named "ffn".
 *   pre = n3 W_1^T + b_1 + s (n3 A_1^T) B_1^T,  act = gelu_tanh(pre)  (one launch);   f = act W_2^T + b_2 + s (act A_2^T) B_2^T
 * `saved` grows by the two down-projected rows [B S, 3r] each and by n3 [B S, D] and act [B S, F], which the frozen base otherwise drops (dA_1 and dA_2 read
 * them).  The backward ADDS to grad_ffn_a1 [r, D], grad_ffn_b1 [F, r], grad_ffn_a2 [r, F], grad_ffn_b2 [D, r] (fp32) as well.  ffn = 0 (ffn_* and grad_ffn_*
 * may then be NULL): none of it -- no launch, no byte.  ffn = 1 needs r > 0 and F >= 256.
 *
 * What the kernels cannot take returns FTMI_ERR_UNSUPPORTED, and the byte planners then return 0 (the reason is in ftmi_last_error).
 * (Until version 100 the library had two narrower entry families next to this one: the same call without TI and ffn, and without ffn.  They issued the
 * launches and planned the bytes of TI = 0, ffn = 0 / of ffn = 0 here and were folded into it at version 101 -- DESIGN.md 7-N; their names are not reused.) */
typedef struct {
    int B, S, T;      /* batch, video tokens, text tokens */
    int D, H, F;      /* width = H x 128 <= 5120, feed-forward width */
    float eps;        /* 1e-6 */
    int gemm_variant; /* 8 */
    int r;            /* LoRA rank: 0, 64 or 128 (other ranks zero-padded by the caller) */
    float lora_scale; /* alpha / (the user's) r */
    int TI;           /* image tokens, 0 .. 320 */
    int ffn;          /* 1: adapters on ffn.net.0.proj and ffn.net.2 as well */
    int TI2;          /* tokens of a second image, 0 .. 320 (first/last-frame); needs TI > 0 */
} ftmi_wan_lora_ffn_block_config;
typedef struct {
    const void* params;                                                          /* flat bf16, WanBlockLayout order */
    const void *w_qkv1_t, *w_o1_t, *w_q2_t, *w_kv2_t, *w_o2_t, *w_f1_t, *w_f2_t; /* transposed twins: backward only */
    const float *lora_a, *lora_b;                                                /* fp32 [8, r, D], [8, D, r]; NULL when r == 0 */
} ftmi_wan_lora_block_weights;
typedef struct {
    ftmi_wan_lora_block_weights base;
    const float *ffn_a1, *ffn_b1, *ffn_a2, *ffn_b2; /* fp32 [r, D], [F, r], [r, F], [D, r]; NULL when ffn == 0 */
} ftmi_wan_lora_ffn_block_weights;
size_t ftmi_wan_lora_ffn_block_saved_bytes(const ftmi_wan_lora_ffn_block_config* cfg);
size_t ftmi_wan_lora_ffn_block_scratch_bytes(const ftmi_wan_lora_ffn_block_config* cfg);
/* out [B, S, D]; out == NULL: recomputation pass (refills `saved`, the feed-forward adapters' rows included) */
int ftmi_wan_lora_ffn_block_forward(const ftmi_wan_lora_ffn_block_config* cfg, const ftmi_wan_lora_ffn_block_weights* w, const void* img_params, const void* x,
                                    const void* enc, const void* enc_img, const float* mod, const float* rope_cos, const float* rope_sin, void* out, void* saved,
                                    size_t saved_bytes, void* scratch, size_t scratch_bytes, ftmi_stream stream);
int ftmi_wan_lora_ffn_block_backward(const ftmi_wan_lora_ffn_block_config* cfg, const ftmi_wan_lora_ffn_block_weights* w, const void* img_params, const void* x,
                                     const void* enc, const void* enc_img, const float* mod, const float* rope_cos, const float* rope_sin, const void* dout,
                                     void* dx, void* denc, float* grad_a, float* grad_b, float* grad_ffn_a1, float* grad_ffn_b1, float* grad_ffn_a2,
                                     float* grad_ffn_b2, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, ftmi_stream stream);

/* Sum of squares of a flat fp32 gradient (shard): scratch[0] <- sum g^2 (order-fixed; scratch >= FTMI_CLIP_SCRATCH_FLOATS floats).  Sharded training
 * all-reduces scratch[0] over the ranks before the optimiser call below (the reference's clip_grad_norm_ over DTensor shards, utils/torch.py:99-161). */
/* n <= 0: FTMI_ERR_INVALID. */
int ftmi_grad_sumsq(const float* grads, long n, float* scratch, ftmi_stream stream);
/* In-place clip of a flat fp32 gradient (shard) by a global norm given as a device sum of squares: grads *= min(1, max_norm / (sqrt(*sumsq) + 1e-6)).
 * The non-stepping micro-steps of a gradient-accumulation window in sharded training (the reference clips after EVERY backward,
 * trainer/sft_trainer/trainer.py:487-492); the stepping micro-step clips inside ftmi_adamw_bf16_step.
 * max_norm <= 0 disables the clip; n == 0: returns 0 without a launch (grad_norm_out not written); n < 0: FTMI_ERR_INVALID. */
int ftmi_clip_by_sumsq(float* grads, long n, const float* sumsq, float max_norm, float* grad_norm_out, ftmi_stream stream);
/* torch.optim.AdamW on bf16 parameters with bf16 moments (the reference's bf16 full fine-tune, optimizer.py:17-46): every torch op of the update is one
 * fp32 computation rounded to bf16.  grads: fp32 (the reduce-scattered shard), multiplied by min(1, max_norm / (sqrt(*sumsq) + 1e-6)) and rounded to
 * bf16 first (sumsq NULL or max_norm <= 0: no clip, the rule of ftmi_clip_adamw_step; a coefficient >= 1 is not applied either).  grad_norm_out
 * (may be NULL) receives sqrt(*sumsq) when sumsq is given.  n == 0: returns 0 without a launch; n < 0: FTMI_ERR_INVALID. */
int ftmi_adamw_bf16_step(void* params, const float* grads, void* exp_avg, void* exp_avg_sq, long n, const float* sumsq, float max_norm, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int step, float* grad_norm_out, ftmi_stream stream);

/* fp32 flat LoRA params (A region [L,8,r,D] then B region [L,8,D,r]) -> the bf16 (hi, lo) working copies of ftmi_ltx_weights */
int ftmi_lora_refresh(const float* a_f32, const float* b_f32, void* lora_a_sp, void* lora_bt_sp, void* lora_b_ext, void* lora_at_ext,
                      void* lora_at_qkv_ext, int L, int r, int D, ftmi_stream stream);
/* the same for a model with n_adapters adapters per block, the first three being q, k, v (CogVideoX: 4) */
int ftmi_lora_refresh_n(const float* a_f32, const float* b_f32, void* lora_a_sp, void* lora_bt_sp, void* lora_b_ext, void* lora_at_ext,
                        void* lora_at_qkv_ext, int L, int n_adapters, int r, int D, ftmi_stream stream);

/* The same split for ONE fp32 matrix w [rows, cols] (building block of ftmi_linear_lora_fwd/_bwd callers): any of the four outputs
 * may be NULL.  sp [2 rows, cols]: (hi, lo) row planes interleaved per 32 rows; ext [rows, 3 cols]: [hi | hi | lo];
 * t_sp [2 cols, rows], t_ext [cols, 3 rows]: the same two layouts of w^T.  sp needs rows % 32 == 0, t_sp cols % 32 == 0 (FTMI_ERR_UNSUPPORTED).
 * rows <= 0 or cols <= 0 (ftmi_lora_refresh_n: L, r or D <= 0): returns 0 without a launch. */
int ftmi_lora_split(const float* w, int rows, int cols, void* sp, void* ext, void* t_sp, void* t_ext, ftmi_stream stream);

/* ftmi_lora_split for `nmat` rectangular fp32 matrices [rows, cols] in ONE launch: matrix m starts at w + m * w_stride (elements; the matrices of one family
 * inside a per-block parameter record, e.g. the A1 of every LTX block), its outputs are packed per matrix in the layouts above (sp / t_sp 2 rows cols apart, ext /
 * t_ext 3 rows cols apart).  What ftmi_lora_refresh_n does for the square attention adapters, for the feed-forward ones of ftmi_ltx_ff_weights: the refresh after
 * an optimiser step (the reference's fp32 adapters need none, trainer/sft_trainer/trainer.py:132-136) is four launches instead of four per block.
 * w_stride >= rows * cols; nmat, rows or cols <= 0: returns 0 without a launch. */
int ftmi_lora_refresh_rect(const float* w, long w_stride, int nmat, int rows, int cols, void* sp, void* ext, void* t_sp, void* t_ext, ftmi_stream stream);

/* ---- Wan control LoRA outside the blocks (csrc/wan_control.hip) ----
 * c [M, N] (fp32, row stride ldc) = (accumulate ? c : 0) + scale * a b, a (m, k) at a[m * lda_row + k * lda_col], b (k, n) at b[k * ldb_row + n * ldb_col]: strides
 * express transposes.  fp32 FMAs, k ascending, one owner per output, no atomics: two runs give the same bits.  hi_lo_out != NULL: the result also as two bf16
 * column planes, hi_lo_out[m * ld_hl + n] = bf(c), hi_lo_out[m * ld_hl + N + n] = bf(c - bf(c)).  M, N, K multiples of 64 (FTMI_ERR_UNSUPPORTED otherwise);
 * c 16-byte aligned with ldc % 4 == 0. */
int ftmi_f32_gemm(int M, int N, int K, const float* a, long lda_row, long lda_col, const float* b, long ldb_row, long ldb_col, float* c, long ldc, float scale,
                  int accumulate, void* hi_lo_out, long ld_hl, ftmi_stream stream);
/* The control specification's input construction in one pass (finetrainers/models/wan/control_specification.py:243-308).  moments [B, 2C, F, H, W] and
 * control_moments [B, 2C, Fc, H, W] bf16 (only the mean halves are read: the posterior's mode), noise [B, C, F, H, W] bf16, sigmas [B] fp32, latents_mean /
 * latents_std [C] fp32 (latents_std is 1 / std: multiplied), keep [B, F] bytes (1 keeps the control frame, 0 drops it; frames >= Fc are zero).
 *   z = bf((mu - mean) * std)      noisy = bf((1 - sigma) * z + sigma * noise)      target [B, C, F, H, W] = bf(noise - z)
 *   cols2 [B S, 2 Kp] = [cols | cols], Kp = 2C pt ph pw, tokens in (f, h, w) order, columns in (c, pt, ph, pw) order: channels 0..C-1 the noisy latents,
 *   channels C..2C-1 bf((mu_c - mean) * std) of a kept control frame, that value times zero for a dropped one, +0 past the control clip. */
typedef struct ftmi_wan_control_pack_config {
    int B, C, F, Fc, H, W;
    int pt, ph, pw;
} ftmi_wan_control_pack_config;
int ftmi_wan_control_pack(const ftmi_wan_control_pack_config* cfg, const void* moments, const void* control_moments, const void* noise, const float* sigmas,
                          const float* latents_mean, const float* latents_std, const unsigned char* keep, void* cols2, void* target, ftmi_stream stream);
/* The full-rank LoRA adapter of the widened patch embedding, folded: y [M, D] = bf(bf(cols W^T + bias) + s (cols A^T) B^T) with fp32 A [r, Kp], B [D, r],
 * computed through dW = s B A (fp32, [D, Kp]) because r >= Kp.
 *   forward : refold != 0: dw_f32 [D, Kp] <- s B A and w2 [D, 2 Kp] <- its bf16 planes [hi | lo] (refold = 0 reuses w2: the parameters did not move);
 *             then ONE NT GEMM: K = Kp over cols2[:, :Kp] and w [D, Kp], K-extension K2 = 2 Kp over cols2 = [cols | cols] and w2, plain store into out.
 *   backward: g_ws [D, Kp] fp32 <- dx0^T cols (zeroed here, one TN GEMM; dx0 [M, D] bf16 = block 0's input gradient), grad_b [D, r] += s g_ws A^T,
 *             grad_a [r, Kp] += s B^T g_ws.  No input gradient: the input is data.
 * FTMI_ERR_UNSUPPORTED for r % 64, Kp % 64 or D % 64. */
typedef struct ftmi_wan_patch_lora_config {
    int M, D, Kp, r;
    float s;
    int gemm_variant;
    int refold;
} ftmi_wan_patch_lora_config;
int ftmi_wan_patch_lora_forward(const ftmi_wan_patch_lora_config* cfg, const void* w, const void* bias, const float* a_f32, const float* b_f32, const void* cols2,
                                float* dw_f32, void* w2, void* out, ftmi_stream stream);
int ftmi_wan_patch_lora_backward(const ftmi_wan_patch_lora_config* cfg, const float* a_f32, const float* b_f32, const void* cols2, const void* dx0, float* g_ws,
                                 float* grad_a, float* grad_b, ftmi_stream stream);

/* ---- Wan latent sampling (csrc/sample_layout.hip, csrc/wan_sample_dit.hip; DESIGN.md "Wan latent sampling") ----
 * The denoising loop of the reference's validation (finetrainers/models/wan/base_specification.py:495-529, control_specification.py:310-377 run a pipeline over
 * the transformer that is being trained) in latent space.  The sampler state lives in the patch embedding's operand layout:
 *   x     fp32 [B, S, Kc]      Kc = C pt ph pw columns in (c, pt, ph, pw) order, S tokens in (f, h, w) order
 *   cols  bf16 [P B S, ld]     the patch-embedding GEMM's operand, ld = copies Kp; columns [0, Kc) of every copy are bf16(x), the others are constant over the loop
 *                              (extra channels, then +0 padding); copies = 2: [cols | cols] as ftmi_wan_control_pack writes it (folded patch adapter);
 *                              P = 2 row groups with guidance (unconditional rows first), 1 without
 *   pred  bf16 [P B, S, po]    as proj_out writes it: po = Kc columns in (pt, ph, pw, c) order
 * FTMI_ERR_UNSUPPORTED: Kc % 8, ld % 8, 2048 % Kc, a latent size that is not whole patches; FTMI_ERR_INVALID: Kc != po, misaligned tensors (16 bytes). */
typedef struct ftmi_wan_sample_geometry {
    int B, C, Cx;   /* samples, latent channels, extra input channels (I2V: 4 mask + 16 condition; control: 16; 0: none) */
    int F, H, W;    /* latent grid */
    int pt, ph, pw; /* patch size */
    int Kp;         /* stored patch width of one copy: >= (C + Cx) pt ph pw */
    int copies;     /* 1, or 2 for [cols | cols] */
    int P;          /* row groups of cols / pred: 2 with guidance, 1 without */
    int po;         /* width of proj_out */
} ftmi_wan_sample_geometry;
/* latents fp32 [B, C, F, H, W], extra bf16 [B, Cx, F, H, W] (NULL when Cx == 0) -> x (the patchified values, exact) and all P row groups and copies of cols. */
int ftmi_wan_sample_init(const ftmi_wan_sample_geometry* geo, const float* latents, const void* extra, float* x, void* cols, ftmi_stream stream);
/* One step: v = fma(g, c - u, u) (guidance == 1: v = c, pred has no unconditional half), x <- fma(sigma_next[b] - sigma[b], v, x) in fp32, bf16(x) into columns
 * [0, Kc) of every row group and copy of cols.  sigma / sigma_next: device fp32 [B].  pred == NULL: only the copies; cols == NULL: only the update. */
int ftmi_wan_sample_step(const ftmi_wan_sample_geometry* geo, const void* pred, float* x, const float* sigma, const float* sigma_next, float guidance, void* cols,
                         ftmi_stream stream);
/* latents bf16 [B, C, F, H, W] = bf16(x * std[c] + mean[c]); std is the VAE's standard deviation itself, NOT the 1 / std the training processors hand over. */
int ftmi_wan_sample_finish(const ftmi_wan_sample_geometry* geo, const float* x, const float* mean, const float* std_, void* latents, ftmi_stream stream);
/* mod fp32 [L, rows, 6, D] = float(tables[l]) + float(tproj): the modulation of all L <= 40 blocks for one step.  tables: HOST array of L device pointers to the
 * blocks' scale_shift_table (bf16 [6 D]); tproj bf16 [6 D]. */
int ftmi_wan_sample_mod(const void* const* tables, int L, const void* tproj, float* mod, int rows, int D, ftmi_stream stream);

/* The whole denoising loop as ONE call, no host synchronisation.  Per step: ftmi_wan_sample_mod; the patch-embedding NT GEMM over cols (patch_fold: the
 * ftmi_wan_patch_lora_forward launch, refolding at step 0 only); L block forwards through ftmi_wan_lora_ffn_block_forward at batch P B (TI = 0: text-to-video, r = 0: no
 * adapters), all blocks sharing ONE `saved` slot and one scratch area, activations alternating between two [P B S, D] buffers; ftmi_wan_ln_fwd with the step's
 * head shift / scale and the proj_out NT GEMM; ftmi_wan_sample_step.  Bit-identical to that composition issued call by call.
 * The caller supplies what does not depend on the state: tproj bf16 [steps, 6 D], head_shift / head_scale fp32 [steps, D], enc bf16 [P B, T, D] (unconditional
 * rows first), enc_img bf16 [P B, TI + TI2, D], the rotary tables fp32 [S, 64], sigmas fp32 [steps + 1] on the device.  The rows of one step share one timestep.
 * x / cols: in and out (ftmi_wan_sample_init wrote them; on return x is the final state and cols its bf16 copies).
 * Workspace: ftmi_wan_sample_workspace_bytes (0 for a refused configuration; it does not depend on L); a smaller one is FTMI_ERR_INVALID. */
typedef struct ftmi_wan_sample_config {
    ftmi_wan_sample_geometry geo;
    int T, TI;          /* text tokens, image tokens (0: none) */
    int D, heads, ffn_dim;
    int L;              /* blocks, 1 .. 40 */
    float eps;          /* 1e-6 */
    int gemm_variant;   /* 8 */
    int r;              /* LoRA rank of the block adapters: 0, 64 or 128 */
    float lora_scale;
    int ffn;            /* 1: adapters on ffn.net.0.proj and ffn.net.2 as well */
    int patch_fold;     /* 1: folded full-rank patch adapter (geo.copies must be 2) */
    int patch_r;        /* its rank */
    float patch_scale;
    int steps;
    float guidance;     /* != 1 needs geo.P == 2 */
    int TI2;            /* tokens of a second image (0: none), handed to the block */
} ftmi_wan_sample_config;
typedef struct ftmi_wan_sample_weights {
    const ftmi_wan_lora_ffn_block_weights* blocks; /* HOST array [L] */
    const void* const* img_params;                 /* HOST array [L] of the blocks' image-context buffers; NULL when TI == 0 */
    const void *patch_w, *patch_b;                 /* bf16 [D, Kp], [D] */
    const void *proj_w, *proj_b;                   /* bf16 [po, D], [po] */
    const float *patch_lora_a, *patch_lora_b;      /* patch_fold: fp32 [patch_r, Kp], [D, patch_r] */
    float* patch_dw;                               /* patch_fold: fp32 [D, Kp], written at step 0 */
    void* patch_w2;                                /* patch_fold: bf16 [D, 2 Kp], written at step 0 */
} ftmi_wan_sample_weights;
size_t ftmi_wan_sample_workspace_bytes(const ftmi_wan_sample_config* cfg);
int ftmi_wan_sample(const ftmi_wan_sample_config* cfg, const ftmi_wan_sample_weights* w, void* cols, float* x, const void* tproj, const float* head_shift,
                    const float* head_scale, const void* enc, const void* enc_img, const float* rope_cos, const float* rope_sin, const float* sigmas,
                    void* workspace, size_t workspace_bytes, ftmi_stream stream);

/* The multistep form of the loop: the scheduler of the Wan2.1 checkpoints, [upstream, unpinned] UniPCMultistepScheduler (flow sigmas, data prediction, bh2,
 * solver_order <= 2), which is what the reference's validation pipeline samples with.  The scheduler is folded on the host into eight numbers per step
 * (finetrainers_amd/wan/sampler.py wan_unipc_tables): coef_row = (c_x, c_l, c_1, c_2, c_t, p_x, p_0, p_1).
 * One step, per element in fp32: v as in ftmi_wan_sample_step; m = fma(-sigma, v, x); x~ = c_x x + c_l last + c_1 m1 + c_2 m2 + c_t m; x' = p_x x~ + p_0 m + p_1 m1
 * (each sum a product, then fmas in this order; a term whose coefficient is 0 is left out and its buffer is not read).  x <- x', last <- x~, m2 <- m (the OLDER
 * history buffer: the caller swaps m1 and m2 after the step), bf16(x') into columns [0, Kc) of every row group and copy of cols (NULL: no copies).
 * last / m1 / m2: fp32 [B, S, Kc] like x, four different buffers; coef_row: device fp32 [8]; sigma: device fp32 [1], the step's sigma (it is not one of the eight
 * numbers: m itself is stored).  Validation and status codes of ftmi_wan_sample_step; pred is required. */
int ftmi_wan_sample_step_unipc(const ftmi_wan_sample_geometry* geo, const void* pred, float* x, float* last, const float* m1, float* m2, const float* coef_row,
                               const float* sigma, float guidance, void* cols, ftmi_stream stream);
/* ftmi_wan_sample's loop with ftmi_wan_sample_step_unipc as the step's last launch; bit-identical to the same launches issued call by call.  coef: device fp32
 * [steps, 8]; sigmas: device fp32 [steps + 1].  The history lives in the workspace: ftmi_wan_sample_ms_workspace_bytes = ftmi_wan_sample_workspace_bytes(base) plus
 * three [B, S, Kc] fp32 buffers (0 for a refused configuration; independent of L).  solver: 1 = UniPC; any other value is FTMI_ERR_UNSUPPORTED. */
typedef struct ftmi_wan_sample_ms_config {
    ftmi_wan_sample_config base;
    int solver;
} ftmi_wan_sample_ms_config;
size_t ftmi_wan_sample_ms_workspace_bytes(const ftmi_wan_sample_ms_config* cfg);
int ftmi_wan_sample_ms(const ftmi_wan_sample_ms_config* cfg, const ftmi_wan_sample_weights* w, void* cols, float* x, const void* tproj, const float* head_shift,
                       const float* head_scale, const void* enc, const void* enc_img, const float* rope_cos, const float* rope_sin, const float* coef,
                       const float* sigmas, void* workspace, size_t workspace_bytes, ftmi_stream stream);

/* ---- CogVideoX latent sampling (csrc/sample_layout.hip: the layout kernels; csrc/cog_dit.hip: the loop) ----
 * The denoising loop of the reference's validation (finetrainers/models/cogvideox/base_specification.py:335-364 runs CogVideoXPipeline over the transformer
 * that is being trained) in latent space, text-to-video: [upstream, unpinned] CogVideoXPipeline + CogVideoXDDIMScheduler (v-prediction, eta = 0).
 * The patch embedding's operand order and proj_out's column order are the same, (c, ph, pw) or (c, pt, ph, pw) with patch_size_t, so the state lives there:
 *   x     fp32 [B, S, Kc]      Kc = C pt p p columns, S = (F / pt)(H / p)(W / p) tokens in (f, h, w) order
 *   cols  bf16 [P B S, Kc]     the patch-embedding GEMM's operand, bf16(x) in every row group; P = 2 with guidance (unconditional rows first), 1 without
 *   pred  bf16 [P B, S, Kc]    as proj_out writes it: the same columns, so a step is a row-major stream with no permutation
 * FTMI_ERR_UNSUPPORTED: Kc % 8, a latent size that is not whole patches, pt > 2; FTMI_ERR_INVALID: empty extents, P, drop, misaligned tensors (16 bytes). */
typedef struct ftmi_cog_sample_geometry {
    int B, C;    /* samples, latent channels */
    int F, H, W; /* latent grid; F counts the frames the pipeline pads at the front (patch_size_t) */
    int p, pt;   /* spatial patch, temporal patch (1: none; 2: CogVideoX 1.5) */
    int P;       /* row groups of cols / pred: 2 with guidance, 1 without */
    int drop;    /* leading frames ftmi_cog_sample_finish leaves out (the pipeline's latents[:, additional_frames:]); 0 <= drop < pt */
} ftmi_cog_sample_geometry;
/* noise fp32 [B, F, C, H, W] -> x (the patchified values, exact) and bf16(x) in all P row groups of cols (replaces the pipeline's prepare_latents hand-over to the
 * transformer's patch embedding, CogVideoXPatchEmbed's reshape / permute per step). */
int ftmi_cog_sample_init(const ftmi_cog_sample_geometry* geo, const float* latents, float* x, void* cols, ftmi_stream stream);
/* One step (replaces the pipeline's noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_uncond) and CogVideoXDDIMScheduler.step): with
 * (cx, cv) = coef[2 step], coef[2 step + 1] read on the device:  d = c - u; v = fma(g, d, u) (guidance == 1: v = c, pred has no unconditional half);
 * x <- fma(cx, x, cv * v) in fp32; bf16(x) into every row group of cols.  pred == NULL: only the copies; cols == NULL: only the update. */
int ftmi_cog_sample_step(const ftmi_cog_sample_geometry* geo, const void* pred, float* x, const float* coef, int step, float guidance, void* cols,
                         ftmi_stream stream);
/* latents bf16 [B, F - drop, C, H, W] = bf16(x * k), the inverse permutation of init without the first `drop` frames (replaces the pipeline's
 * latents[:, additional_frames:] and decode_latents' 1 / scaling_factor; k = scaling_factor for the invert_scale_latents checkpoints). */
int ftmi_cog_sample_finish(const ftmi_cog_sample_geometry* geo, const float* x, float k, void* latents, ftmi_stream stream);

/* The whole denoising loop as ONE call, no host synchronisation (replaces the loop of CogVideoXPipeline.__call__ the reference's validation drives,
 * base_specification.py:335-364).  Before the loop the text projection writes the text rows of tokens_in [P B, T + S, D] once.  Per step: the patch-embedding
 * NT GEMM over cols into the video rows of tokens_in (one launch per model row, as the model's forward issues them); pos != NULL: + the sincos table
 * (ftmi_cog_gate_residual); the block walk of ftmi_cog_blocks_forward at batch P B over a forward-only layout (every block writes the same slot, the hidden
 * state alternates between two buffers); norm_final on the video rows; norm_out with the step's shift / 1 + scale; proj_out; ftmi_cog_sample_step.
 * Bit-identical to that composition issued call by call.
 * The caller supplies what does not depend on the state: text bf16 [P B, T, D_text] (unconditional rows first), temb_silu bf16 [steps, P B, D_temb],
 * head_shift / head_onep bf16 [steps, D], coef fp32 [steps, 2] on the device, the rotary tables in blocks.rope_cos / rope_sin.
 * x / cols: in and out (ftmi_cog_sample_init wrote them).  Workspace: ftmi_cog_sample_workspace_bytes (0 for a refused configuration; it depends on L only
 * through the modulation tables); a smaller one is FTMI_ERR_INVALID. */
typedef struct ftmi_cog_sample_config {
    ftmi_cog_sample_geometry geo;
    int T, D_text;            /* text tokens, width of the text embeddings */
    int D, heads, L;          /* width = heads x 64, blocks */
    int D_ff, D_temb;
    int r;                    /* LoRA rank (0: none; multiple of 64) */
    float lora_scale, eps_norm, eps_qk;
    int gemm_variant;         /* 8 */
    int steps;
    float guidance;           /* != 1 needs geo.P == 2 */
} ftmi_cog_sample_config;
typedef struct ftmi_cog_sample_weights {
    ftmi_cog_weights blocks;                      /* the "_t" copies and the backward's adapter copies are not read */
    const void *patch_w, *patch_b;                /* bf16 [D, Kc], [D] */
    const void *text_w, *text_b;                  /* bf16 [D, D_text], [D] */
    const void* pos;                              /* bf16 [T + S, D]: the sincos table, text rows zero; NULL for the rotary checkpoints */
    const void *norm_final_w, *norm_final_b;      /* bf16 [D] */
    const void *norm_out_w, *norm_out_b;          /* bf16 [D] */
    const void *proj_w, *proj_b;                  /* bf16 [Kc, D], [Kc] */
    const void *ones, *zeros;                     /* bf16 [D] of 1 and of 0 (the unmodulated norm_final, the position table's unit gate) */
} ftmi_cog_sample_weights;
size_t ftmi_cog_sample_workspace_bytes(const ftmi_cog_sample_config* cfg);
int ftmi_cog_sample(const ftmi_cog_sample_config* cfg, const ftmi_cog_sample_weights* w, void* cols, float* x, const void* text, const void* temb_silu,
                    const void* head_shift, const void* head_onep, const float* coef, void* workspace, size_t workspace_bytes, ftmi_stream stream);

/* The multistep form of the loop: the scheduler of the CogVideoX-5b and CogVideoX1.5-5B checkpoints, [upstream, unpinned] CogVideoXDPMScheduler (v-prediction,
 * trailing spacing), a second-order multistep SDE solver: it keeps the previous step's x0 prediction and adds fresh Gaussian noise at every step but the last.
 * The scheduler is folded on the host into eight numbers per step (finetrainers_amd/cogvideox/sampler.py cog_dpm_tables):
 * coef_row = (sa, sb, m0, e0, e1, mn, g, 0), g the step's guidance scale (use_dynamic_cfg changes it per step).
 * One step, per element in fp32, the row read on the device: v as in ftmi_cog_sample_step with g = coef_row[6] (geo.P == 1: v = c);
 * x0 = fma(-sb, v, sa x); x' = m0 x; x' = fma(e0, x0, x'); e1 != 0: x' = fma(e1, old, x'); mn != 0: x' = fma(mn, z, x').  x <- x', old <- x0, bf16(x') into
 * every row group of cols (NULL: no copies).  A term whose coefficient is 0 is left out and its buffer is not read: old may hold anything at step 0, noise may
 * be NULL when mn == 0 (a NULL noise is read as mn == 0).  old fp32 [B, S, Kc] like x; noise fp32 [B, S, Kc], the step's slice in the state's layout
 * (ftmi_cog_sample_pack); x, old and noise are three buffers.  Validation, alignment rules and status codes of ftmi_cog_sample_step; pred is required. */
int ftmi_cog_sample_step_dpm(const ftmi_cog_sample_geometry* geo, const void* pred, float* x, float* old, const float* noise, const float* coef_row, void* cols,
                             ftmi_stream stream);
/* latents fp32 [n, B, F, C, H, W] -> out fp32 [n, B, S, Kc]: the permutation of ftmi_cog_sample_init over n tensors at once, values exact, no cols. */
int ftmi_cog_sample_pack(const ftmi_cog_sample_geometry* geo, const float* latents, int n, float* out, ftmi_stream stream);
/* ftmi_cog_sample's loop with ftmi_cog_sample_step_dpm as the step's last launch; bit-identical to the same launches issued call by call.  coef: device fp32
 * [steps, 8]; noise: device fp32 [noise_steps, B, S, Kc], the slices of the leading noise_steps steps (0 .. steps; the caller passes steps - 1 when the last row
 * has mn == 0, 0 and NULL when no row has noise); a step past them runs without noise.  noise != NULL exactly when noise_steps > 0, else FTMI_ERR_INVALID.
 * base.guidance only decides P (!= 1 exactly when geo.P == 2): the scale of a step is its row's.  The history lives in the workspace:
 * ftmi_cog_sample_ms_workspace_bytes = ftmi_cog_sample_workspace_bytes(base) plus ONE [B, S, Kc] fp32 buffer (0 for a refused configuration).
 * solver: 1 = DPM; any other value is FTMI_ERR_UNSUPPORTED. */
typedef struct ftmi_cog_sample_ms_config {
    ftmi_cog_sample_config base;
    int solver;
} ftmi_cog_sample_ms_config;
size_t ftmi_cog_sample_ms_workspace_bytes(const ftmi_cog_sample_ms_config* cfg);
int ftmi_cog_sample_ms(const ftmi_cog_sample_ms_config* cfg, const ftmi_cog_sample_weights* w, void* cols, float* x, const void* text, const void* temb_silu,
                       const void* head_shift, const void* head_onep, const float* coef, const float* noise, int noise_steps, void* workspace,
                       size_t workspace_bytes, ftmi_stream stream);

/* ---- HunyuanVideo latent sampling (csrc/sample_layout.hip: the layout kernels; csrc/hy_sample_dit.hip: the loop) ----
 * The denoising loop of the reference's validation (finetrainers/models/hunyuan_video/base_specification.py:332-355 runs HunyuanVideoPipeline over the
 * transformer that is being trained) in latent space, text-to-video: [upstream, unpinned] HunyuanVideoPipeline + FlowMatchEulerDiscreteScheduler (static
 * shift 7, embedded guidance; optional true classifier-free guidance over a negative prompt).
 * The patch embedding's operand order and proj_out's column order are the same, (c, pt, ph, pw), so the state lives there as for CogVideoX:
 *   x     fp32 [B, S, Kc]      Kc = C pt p p columns (64 for the checkpoint), S = (F / pt)(H / p)(W / p) tokens in (f, h, w) order
 *   cols  bf16 [P B S, Kc]     the patch-embedding GEMM's operand, bf16(x) in every row group; P = 2 with true CFG (unconditional rows first), 1 without
 *   pred  bf16 [P B, S, Kc]    as proj_out writes it: the same columns, so a step is a row-major stream with no permutation
 * FTMI_ERR_UNSUPPORTED: Kc % 8, a latent size that is not whole patches; FTMI_ERR_INVALID: empty extents, P, misaligned tensors (16 bytes). */
typedef struct ftmi_hy_sample_geometry {
    int B, C;    /* samples, latent channels */
    int F, H, W; /* latent grid */
    int p, pt;   /* spatial patch, temporal patch (1 for every published checkpoint) */
    int P;       /* row groups of cols / pred: 2 with true CFG, 1 without */
} ftmi_hy_sample_geometry;
/* noise fp32 [B, C, F, H, W] -> x (the patchified values, exact) and bf16(x) in all P row groups of cols (replaces the pipeline's prepare_latents hand-over
 * and the transformer's per-step Conv3d patchify). */
int ftmi_hy_sample_init(const ftmi_hy_sample_geometry* geo, const float* latents, float* x, void* cols, ftmi_stream stream);
/* One step (replaces the pipeline's neg + true_cfg_scale * (noise_pred - neg) and FlowMatchEulerDiscreteScheduler.step): dt = sigmas[step + 1] - sigmas[step]
 * read on the device from the fp32 table [steps + 1];  d = c - u; v = fma(g, d, u) (true_cfg == 1: v = c, pred has no unconditional half);
 * x <- fma(dt, v, x) in fp32; bf16(x) into every row group of cols.  pred == NULL: only the copies; cols == NULL: only the update. */
int ftmi_hy_sample_step(const ftmi_hy_sample_geometry* geo, const void* pred, float* x, const float* sigmas, int step, float true_cfg, void* cols,
                        ftmi_stream stream);
/* latents bf16 [B, C, F, H, W] = bf16(x * k), the inverse permutation of init (replaces the pipeline's latents / vae.config.scaling_factor; k = 1 / it). */
int ftmi_hy_sample_finish(const ftmi_hy_sample_geometry* geo, const float* x, float k, void* latents, ftmi_stream stream);

/* The whole denoising loop as ONE call, no host synchronisation (replaces the loop of HunyuanVideoPipeline.__call__ the reference's validation drives,
 * base_specification.py:332-355).  Per step, the launches of MI355XHunyuanVideoTransformer3DModel.forward at batch P B, in its order: the patch-embedding NT
 * GEMM over cols; Ld dual-stream blocks through ftmi_hy_dual_forward (one call per sample row, the streams alternating between two buffers each, the last one
 * writing into the rows of the joint buffer [P B, T + S, D], text first); Ls single-stream blocks through ftmi_hy_single_forward at batch P B over two joint
 * buffers; ftmi_cog_ln_mod_fwd on the video rows with the step's per-row shift / 1 + scale (no affine); the proj_out NT GEMM; ftmi_hy_sample_step.  Every
 * block writes the same `saved` slot and shares one scratch area: nothing in the workspace grows with Ld or Ls.  Bit-identical to that composition.
 * fp8 storage: upcasts != NULL lists, per block (dual blocks first), what ftmi_fp8_upcast has to write into `arena` right before the block's launches;
 * upcast_count[l] entries belong to block l.  The block structures then point into the arena.  NULL: bf16 weights.
 * The caller supplies what does not depend on the state: temb_silu bf16 [steps, P B, D] = silu(conditioning vector), enc bf16 [steps, P B, T, D] (the refined
 * text depends on the timestep), head_shift / head_onep bf16 [steps, P B, D], key_bias fp32 [P B, T + S] (-inf on padded text keys) or NULL, the rotary tables
 * fp32 [S, 128], sigmas fp32 [steps + 1] on the device.  x / cols: in and out (ftmi_hy_sample_init wrote them).  Workspace:
 * ftmi_hy_sample_text_workspace_bytes (0 for a refused configuration); a smaller one is FTMI_ERR_INVALID. */
typedef struct ftmi_hy_sample_upcast {
    const void* src;  /* fp8 e4m3fn [rows, cols] */
    int rows, cols;
    size_t offset;    /* bf16 elements from the start of the arena */
} ftmi_hy_sample_upcast;
typedef struct ftmi_hy_sample_config {
    ftmi_hy_sample_geometry geo;
    int T;                    /* text tokens */
    int D, H, mlp;            /* width = H x 128, feed-forward width */
    int Ld, Ls;               /* dual-stream, single-stream blocks */
    int r;                    /* LoRA rank (0: none; multiple of 64) */
    float lora_scale, eps;
    int gemm_variant;         /* 8 */
    int steps;
    float true_cfg;           /* != 1 needs geo.P == 2 */
} ftmi_hy_sample_config;
typedef struct ftmi_hy_sample_weights {
    const ftmi_hy_dual_weights* dual;        /* HOST array [Ld]; the "_t" copies are not read */
    const ftmi_hy_single_weights* single;    /* HOST array [Ls] */
    const ftmi_hy_sample_upcast* upcasts;    /* HOST array, block after block; NULL: bf16 weights */
    const int* upcast_count;                 /* HOST array [Ld + Ls] */
    void* arena;                             /* bf16, device */
    const void *patch_w, *patch_b;           /* bf16 [D, Kc], [D] */
    const void *proj_w, *proj_b;             /* bf16 [Kc, D], [Kc] */
    const void *ones, *zeros;                /* bf16 [D] of 1 and of 0 (the affine-free output norm) */
} ftmi_hy_sample_weights;
/* What the loop takes: `base` as above, then text_adapters as in ftmi_hy_dual_config (0: the video stream's adapters alone; 1: every dual block's lora_a /
 * lora_b hold 8 matrices, the text stream's adapters as well; needs base.r > 0; other values than 0 / 1 are FTMI_ERR_INVALID, a workspace size of 0).  The flag
 * is handed to every ftmi_hy_dual_forward of the walk and the workspace follows that block's layout. */
typedef struct ftmi_hy_sample_text_config {
    ftmi_hy_sample_config base;
    int text_adapters;        /* 0 or 1 */
} ftmi_hy_sample_text_config;
size_t ftmi_hy_sample_text_workspace_bytes(const ftmi_hy_sample_text_config* cfg);
int ftmi_hy_sample_text(const ftmi_hy_sample_text_config* cfg, const ftmi_hy_sample_weights* w, void* cols, float* x, const void* temb_silu, const void* enc,
                        const void* head_shift, const void* head_onep, const float* key_bias, const float* rope_cos, const float* rope_sin, const float* sigmas,
                        void* workspace, size_t workspace_bytes, ftmi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* FTMI355_H */
