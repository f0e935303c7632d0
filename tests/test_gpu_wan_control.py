"""Wan control LoRA on the GPU (``--training_type control-lora``): the pack kernel against the eager restatement bit for bit, the fp32 GEMM against fp64, the
folded full-rank patch-embedding adapter against its fp64 evaluation and the reference-dtype restatement, then model, step and specification against
tests/wan_control_reference.py (oracle.wan with the widened patch embedding and peft's conv adapter)."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
SMALL = dict(num_attention_heads=2, attention_head_dim=128, ffn_dim=512, text_dim=64)
D = 256
RECIPE = "(^patch_embedding$)|(blocks.*(to_q|to_k|to_v|to_out.0|ff.net.0.proj|ff.net.2))"  # what the control trainer passes for the recipe's --target_modules
PATTERN = {"patch_embedding": D}


def _dev():
    return torch.device("cuda", 0)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- pack kernel ---------------------------------------------------------------------------------------------------------------------------------------
def _pack_batch(F_, H, W, Fc, seed, B=2, C=16):
    g = torch.Generator().manual_seed(seed)
    moments = torch.randn(B, 2 * C, F_, H, W, generator=g).to(bf16)
    control = torch.randn(B, 2 * C, Fc, H, W, generator=g).to(bf16)
    noise = torch.randn(B, C, F_, H, W, generator=g).to(bf16)
    return dict(moments=moments, control=control, noise=noise, sigmas=torch.tensor([0.23, 0.81][:B]), mean=0.1 * torch.randn(C, generator=g),
                std=1.0 + 0.2 * torch.rand(C, generator=g))


def _keep(kind, B, F_, Fc):
    n = min(F_, Fc)
    k = torch.zeros(B, F_, dtype=torch.uint8)
    if kind == "all":
        k[:, :n] = 1
    elif kind == "frame0":
        k[:, 0] = 1
    elif kind == "first_and_last":
        k[:, 0] = 1
        k[:, n - 1] = 1
    return k


@pytest.mark.parametrize("kind", ["all", "frame0", "first_and_last", "none"])
@pytest.mark.parametrize("Fc", [1, 3])
@pytest.mark.parametrize("F_,H,W", [(3, 4, 6), (1, 2, 2)])
def test_control_pack_is_the_eager_graph_bit_for_bit(F_, H, W, Fc, kind):
    """18 tokens per sample and a single token; control clips shorter than, as long as and longer than the latents; two sigmas in the batch.  Both halves of
    cols2 and the target carry the restatement's bits -- the sign of a dropped frame's zero included."""
    import wan_control_reference as ref
    from finetrainers_amd import ops

    b = _pack_batch(F_, H, W, Fc, seed=F_ * 100 + Fc)
    keep = _keep(kind, 2, F_, Fc)
    cols2_ref, target_ref = ref.pack_reference(b["moments"], b["control"], b["mean"], b["std"], b["sigmas"], b["noise"], keep)
    dev = _dev()
    cols2, target = ops.wan_control_pack(b["moments"].to(dev), b["control"].to(dev), b["noise"].to(dev), b["sigmas"].to(dev), b["mean"].to(dev), b["std"].to(dev),
                                         keep.to(dev))
    torch.cuda.synchronize()
    S = F_ * (H // 2) * (W // 2)
    assert cols2.shape == (2 * S, 256) and cols2.dtype == bf16 and target.shape == b["noise"].shape
    assert torch.equal(_bits(cols2.cpu()), _bits(cols2_ref)), "cols2"
    assert torch.equal(_bits(cols2[:, :128].cpu()), _bits(cols2[:, 128:].cpu()))
    assert torch.equal(_bits(target.cpu()), _bits(target_ref)), "target"
    if kind == "none":
        assert float(cols2[:, 64:128].float().abs().max()) == 0.0


# ---- fp32 GEMM -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(64, 64, 64), (256, 128, 320), (128, 256, 192)])
def test_f32_gemm_against_fp64(M, N, K):
    """Plain, both transposed and an unaligned operand layout, accumulate 0 / 1, scale 1 and != 1.  Each element within (K + 1) 2^-24 sum |a| |b| of fp64 -- the bound of an
    fp32 dot product of that length (the accumulated-into value counts as one more term); an fp32 torch.matmul on the CPU stays inside it on these inputs.
    The bf16 planes add up to the result to 2^-16 |c|; two runs give identical bits."""
    from finetrainers_amd import ops

    dev = _dev()
    g = torch.Generator().manual_seed(M + N + K)
    u = 2.0 ** -24
    for layout in ("plain", "a_t", "b_t", "unaligned"):
        a = torch.randn(M, K, generator=g)
        b = torch.randn(K, N, generator=g)
        c0 = torch.randn(M, N, generator=g)
        ag = a.t().contiguous().to(dev).t() if layout == "a_t" else a.to(dev)
        bg = b.t().contiguous().to(dev).t() if layout == "b_t" else b.to(dev)
        if layout == "unaligned":  # views one float into wider buffers: rows that start off the 16-byte grid take the kernel's scalar loads
            ag, bg = torch.zeros(M, K + 3, device=dev)[:, 1:K + 1].copy_(ag), torch.zeros(K, N + 3, device=dev)[:, 1:N + 1].copy_(bg)
            assert ag.data_ptr() % 16 == 4 and bg.data_ptr() % 16 == 4 and ag.stride(0) == K + 3
        assert ag.shape == (M, K) and bg.shape == (K, N) and (ag.stride(1) == 1) == (layout != "a_t") and (bg.stride(1) == 1) == (layout != "b_t")
        mag = a.double().abs() @ b.double().abs()
        for accumulate in (False, True):
            for scale in (1.0, -0.625):
                want = scale * (a.double() @ b.double()) + (c0.double() if accumulate else 0.0)
                bound = (K + 1) * u * (abs(scale) * mag + (c0.double().abs() if accumulate else 0.0))
                host = scale * (a @ b) + (c0 if accumulate else 0.0)  # fp32 on the CPU
                assert bool(((host.double() - want).abs() <= bound).all()), "the bound does not hold for an fp32 matmul: the test's own bound is wrong"
                outs = []
                for _ in range(2):
                    out = c0.to(dev).clone() if accumulate else torch.full((M, N), float("nan"), device=dev)
                    hl = torch.zeros(M, 2 * N, dtype=bf16, device=dev)
                    ops.f32_gemm(ag, bg, out=out, scale=scale, accumulate=accumulate, hi_lo=hl)
                    outs.append((out.cpu(), hl.cpu()))
                (c, hl), (c2, hl2) = outs
                err = (c.double() - want).abs()
                worst = float((err / bound).max())
                print(f"[f32_gemm {M}x{N}x{K} {layout} acc={int(accumulate)} scale={scale}] worst error / bound {worst:.3f}; rel {_rel(c, want):.2e} (cpu fp32 {_rel(host, want):.2e})")
                assert bool((err <= bound).all()), (layout, accumulate, scale, worst)
                assert torch.equal(c, c2) and torch.equal(_bits(hl), _bits(hl2)), "two runs differ"
                planes = hl[:, :N].float() + hl[:, N:].float()
                assert bool(((planes - c).abs() <= 2.0 ** -16 * c.abs()).all())


def test_f32_gemm_refuses_what_it_does_not_tile():
    from finetrainers_amd import ops

    dev = _dev()
    with pytest.raises(ValueError):
        ops.f32_gemm(torch.zeros(64, 96, device=dev), torch.zeros(96, 64, device=dev))
    with pytest.raises(ValueError):
        ops.f32_gemm(torch.zeros(32, 64, device=dev), torch.zeros(64, 64, device=dev))


# ---- the folded patch adapter, C call --------------------------------------------------------------------------------------------------------------------
def _adapter_case(M, Dm, seed, Kp=128):
    g = torch.Generator().manual_seed(seed)
    cols = torch.randn(M, Kp, generator=g).to(bf16)
    w = (torch.randn(Dm, Kp, generator=g) / Kp ** 0.5).to(bf16)
    bias = (0.05 * torch.randn(Dm, generator=g)).to(bf16)
    a = (torch.rand(Dm, Kp, generator=g) * 2 - 1) / Kp ** 0.5
    b = 0.05 * torch.randn(Dm, Dm, generator=g)
    dy = torch.randn(M, Dm, generator=g).to(bf16)
    return cols, w, bias, a, b, dy


def _run_adapter(cols, w, bias, a, b, dy, s=1.0):
    from finetrainers_amd import ops

    dev = _dev()
    Dm, Kp = w.shape
    cols2 = torch.cat([cols, cols], dim=1).to(dev)
    ag, bg = a.to(dev), b.to(dev)
    dw, w2, gws = torch.empty(Dm, Kp, device=dev), torch.empty(Dm, 2 * Kp, dtype=bf16, device=dev), torch.empty(Dm, Kp, device=dev)
    y = ops.wan_patch_lora_forward(cols2, w.to(dev), bias.to(dev), ag, bg, dw, w2, s=s, refold=True)
    y_again = ops.wan_patch_lora_forward(cols2, w.to(dev), bias.to(dev), ag, bg, dw, w2, s=s, refold=False)
    ga, gb = torch.zeros_like(ag), torch.zeros_like(bg)
    ops.wan_patch_lora_backward(cols2, dy.to(dev), ag, bg, gws, ga, gb, s=s)
    torch.cuda.synchronize()
    assert torch.equal(y, y_again), "refold = 0 must reuse the planes"
    return y.cpu(), ga.cpu(), gb.cpu(), dw.cpu()


@pytest.mark.parametrize("M", [18, 200])
@pytest.mark.parametrize("Dm", [256, 384])
def test_patch_adapter_against_fp64_and_the_reference_dtypes(Dm, M):
    """y, grad_A, grad_B: the kernel path's distance from the fp64 evaluation is at most 2.0 x that of the eager restatement in the reference's dtypes (bf16
    base, fp32 adapter branch, the two roundings), in relative Frobenius norm -- the ratio this project holds its kernels to."""
    import wan_control_reference as ref

    cols, w, bias, a, b, dy = _adapter_case(M, Dm, seed=Dm + M)
    y64, ga64, gb64 = ref.patch_adapter_fp64(cols, w, bias, a, b, 1.0, dy)
    ye, gae, gbe = ref.patch_adapter_eager(cols, w, bias, a, b, 1.0, dy)
    y, ga, gb, dw = _run_adapter(cols, w, bias, a, b, dy)
    assert _rel(dw, b.double() @ a.double()) < 1e-6
    for name, got, eager, want in (("y", y, ye, y64), ("grad_A", ga, gae, ga64), ("grad_B", gb, gbe, gb64)):
        e_k, e_e = _rel(got, want), _rel(eager, want)
        print(f"[patch adapter D=r={Dm} M={M}] {name}: kernel vs fp64 {e_k:.3e}, eager vs fp64 {e_e:.3e}, ratio {e_k / e_e:.2f}")
        assert e_k <= 2.0 * e_e, (name, e_k, e_e)


@pytest.mark.parametrize("M", [18, 200])
@pytest.mark.parametrize("Dm", [256, 384])
def test_patch_adapter_with_zero_b_is_the_plain_layer(Dm, M):
    """peft's initialisation: y has the bits of the plain GEMM without extension, grad_A is exactly zero, grad_B is not."""
    from finetrainers_amd import ops

    cols, w, bias, a, b, dy = _adapter_case(M, Dm, seed=Dm + M + 1)
    y, ga, gb, dw = _run_adapter(cols, w, bias, a, torch.zeros_like(b), dy)
    dev = _dev()
    plain = ops.gemm_nt(cols.to(dev), w.to(dev), bias.to(dev)).cpu()
    assert torch.equal(_bits(y), _bits(plain)), f"{_rel(y, plain):.2e}"
    assert float(ga.abs().max()) == 0.0 and float(dw.abs().max()) == 0.0 and float(gb.abs().max()) > 0.0


# ---- model -------------------------------------------------------------------------------------------------------------------------------------------------
def _fix(k):
    return k.replace("ffn.proj_in.", "ffn.net.0.proj.").replace("ffn.proj_out.", "ffn.net.2.")


def _lora_keys(model):
    return {n.replace(".default.", "."): p for n, p in model.named_parameters() if "lora_" in n}


def _model_pair(layers=2, rank=32, alpha=32.0, seed=0, patch=True, patch_b_std=0.02):
    """(oracle model: 32-channel patch embedding with peft's conv adapter at r = D, alpha = D, LoraLinear on the eight attention projections of every block;
    the MI355X model with the same base weights and adapters)."""
    import wan_control_reference as ref
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig
    from oracle import ltx, wan

    torch.manual_seed(seed)
    omodel = wan.WanTransformer3DModel(wan.WanConfig(num_layers=layers, **SMALL))
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in omodel.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    omodel = omodel.to(bf16)
    gmodel = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, **SMALL), device=_dev())
    gmodel.load_diffusers_state_dict({_fix(k): v for k, v in omodel.state_dict().items()})
    gmodel.expand_patch_embedding(32)
    omodel.patch_embedding = ref.expand_conv3d(omodel.patch_embedding, 32)
    for p in omodel.parameters():
        p.requires_grad_(False)
    for blk in omodel.blocks:
        for attn in (blk.attn1, blk.attn2):
            for t in ("to_q", "to_k", "to_v"):
                setattr(attn, t, ltx.LoraLinear(getattr(attn, t), rank, alpha))
            attn.to_out[0] = ltx.LoraLinear(attn.to_out[0], rank, alpha)
    if patch:
        omodel.patch_embedding = ref.LoraConv3d(omodel.patch_embedding, D, float(D))
    with torch.no_grad():  # the blocks first: the same block adapters with and without the patch adapter
        for n, p in omodel.named_parameters():
            if "lora_B" in n and not n.startswith("patch_embedding"):
                p.normal_(0, 0.02, generator=g)
        if patch and patch_b_std > 0:
            omodel.patch_embedding.lora_B["default"].weight.normal_(0, patch_b_std, generator=g)
    if patch:
        gmodel.add_adapter(rank, alpha, target_modules=RECIPE, rank_pattern=PATTERN, alpha_pattern=PATTERN)
    else:
        gmodel.add_adapter(rank, alpha, target_modules=["to_q", "to_k", "to_v", "to_out.0", "^patch_embedding$"], rank_pattern=PATTERN, alpha_pattern=PATTERN)
    gmodel.load_lora_state_dict({k: v.detach() for k, v in _lora_keys(omodel).items()})
    return omodel, gmodel


def _batch(B=2, seed=11, Fc=2):
    g = torch.Generator().manual_seed(seed)
    C, F_, H, W = 16, 2, 8, 12  # 2 x 4 x 6 = 48 tokens
    b = dict(moments=torch.randn(B, 2 * C, F_, H, W, generator=g).to(bf16), control=torch.randn(B, 2 * C, Fc, H, W, generator=g).to(bf16),
             text=torch.randn(B, 16, 64, generator=g).to(bf16), noise=torch.randn(B, C, F_, H, W, generator=g).to(bf16), sigmas=torch.tensor([0.23, 0.81][:B]),
             mean=0.1 * torch.randn(C, generator=g), std=1.0 + 0.2 * torch.rand(C, generator=g))
    b["keep"] = torch.tensor([[1, 0]] * B, dtype=torch.uint8)  # the recipe: index conditioning on frame 0
    return b


def _oracle_run(model, cast, b):
    import wan_control_reference as ref
    from oracle import wan

    for p in model.parameters():
        p.grad = None
    pred, target, _ = ref.spec_forward_control(model, b["moments"].to(cast), b["control"].to(cast), b["mean"], b["std"], b["text"].to(cast), b["sigmas"],
                                               b["noise"].to(cast), b["keep"])
    loss = wan.sft_loss(pred, target, b["sigmas"])
    loss.backward()
    return loss.item(), pred.detach(), {k: p.grad.detach().clone() for k, p in _lora_keys(model).items()}


def _gpu_run(gmodel, b, **kw):
    from finetrainers_amd.wan import MI355XWanControlSpecOps

    dev = _dev()
    spec = MI355XWanControlSpecOps()
    for p in gmodel.lora_parameters():
        p.grad = None
    pred, target, _ = spec.forward(gmodel, b["moments"].to(dev), b["text"].to(dev), b["sigmas"].to(dev), b["mean"].to(dev), b["std"].to(dev), noise=b["noise"].to(dev),
                                   control_latents=b["control"].to(dev), keep=b["keep"], **kw)
    loss = spec.loss_backward(pred, target)
    torch.cuda.synchronize()
    return loss.item(), pred.detach().clone(), target.detach().clone(), {k: v.detach().cpu().clone() for k, v in gmodel.lora_grad_state_dict().items()}


@pytest.fixture(scope="module")
def parity():
    """One oracle evaluation (bf16 restatement and its fp32 evaluation) shared by the model tests."""
    omodel, gmodel = _model_pair()
    b = _batch()
    loss_ref, pred_ref, g_ref = _oracle_run(omodel, bf16, b)
    loss32, pred32, g32 = _oracle_run(copy.deepcopy(omodel).float(), torch.float32, b)
    return dict(gmodel=gmodel, b=b, ref=(loss_ref, pred_ref, g_ref), f32=(loss32, pred32, g32))


def test_control_model_parity(parity):
    """Two blocks, 32 input channels, rank-32 block adapters and the full-rank patch adapter: pred and every adapter gradient within test_lora_block_parity's
    bounds against the bf16 restatement and its fp32 evaluation; the patch adapter's two gradients within 2.0 x the restatement's own distance from fp32."""
    from oracle import ltx

    (loss_ref, pred_ref, g_ref), (loss32, pred32, g32) = parity["ref"], parity["f32"]
    loss, pred, _, got = _gpu_run(parity["gmodel"], parity["b"])
    assert set(got) == set(g_ref) and len(got) == 2 * 16 + 2
    assert got["patch_embedding.lora_A.weight"].shape == (D, 32, 1, 2, 2) and got["patch_embedding.lora_B.weight"].shape == (D, D, 1, 1, 1)
    floor, floor_worst = ltx.grads_rel_l2(g_ref, g32)
    glob, worst = ltx.grads_rel_l2(got, g_ref)
    glob32, worst32 = ltx.grads_rel_l2(got, g32)
    e_pred = _rel(pred, pred_ref)
    print(f"[wan-control model] pred {e_pred:.2e} (restatement bf16 vs fp32 {_rel(pred_ref, pred32):.2e}) loss {loss:.6f} vs {loss_ref:.6f} (fp32 {loss32:.6f}) | "
          f"adapter gradients vs bf16 restatement {glob:.2e} (worst {worst:.2e}), vs fp32 {glob32:.2e} (worst {worst32:.2e}); restatement bf16 vs fp32 {floor:.2e} "
          f"(worst {floor_worst:.2e})")
    assert e_pred < 5e-3
    assert glob < 2.0 * floor + 2e-3 and worst < 2.0 * floor_worst + 5e-3
    assert glob32 < 1.5 * floor + 1e-3 and worst32 < 1.5 * floor_worst + 2e-3
    for k in ("patch_embedding.lora_A.weight", "patch_embedding.lora_B.weight"):
        e_k, e_e = _rel(got[k], g32[k]), _rel(g_ref[k], g32[k])
        print(f"[wan-control model] {k}: kernel vs fp32 {e_k:.3e}, bf16 restatement vs fp32 {e_e:.3e}, ratio {e_k / e_e:.2f}")
        assert e_k <= 2.0 * e_e, (k, e_k, e_e)
        assert float(got[k].abs().max()) > 0.0


def test_zero_patch_b_gives_the_bits_of_the_model_without_the_patch_adapter():
    _, with_patch = _model_pair(patch_b_std=0.0)
    _, without = _model_pair(patch=False)
    assert with_patch.patch_lora_A is not None and without.patch_lora_A is None and without.config.in_channels == 32
    assert float(with_patch.patch_lora_B.detach().abs().max()) == 0.0
    b = _batch()
    _, pred1, _, g1 = _gpu_run(with_patch, b)
    _, pred0, _, g0 = _gpu_run(without, b, use_pack_kernel=False)
    assert torch.equal(_bits(pred1), _bits(pred0)), f"{_rel(pred1, pred0):.2e}"
    assert float(g1["patch_embedding.lora_A.weight"].abs().max()) == 0.0 and float(g1["patch_embedding.lora_B.weight"].abs().max()) > 0.0


def test_checkpointing_and_the_python_walk_agree(parity):
    """Gradient checkpointing: same forward bits, gradients within the 2e-6 of the existing recompute tests (the order of the fp32 atomics).  The native block
    path against the per-kernel composition from Python (FTMI_NATIVE_BLOCKS=0): as today, prediction bit-equal, gradients within 2e-6."""
    gmodel, b = parity["gmodel"], parity["b"]
    loss0, pred0, _, g0 = _gpu_run(gmodel, b)
    try:
        for blk in gmodel.blocks:
            blk.native = False
        loss2, pred2, _, g2 = _gpu_run(gmodel, b)
    finally:
        for blk in gmodel.blocks:
            blk.native = True
    gmodel.apply_activation_checkpointing()
    try:
        loss1, pred1, _, g1 = _gpu_run(gmodel, b)
    finally:
        for blk in gmodel.blocks:
            blk.gradient_checkpointing = False
    assert loss0 == loss1 == loss2 and torch.equal(pred0, pred1) and torch.equal(pred0, pred2)
    for tag, other in (("checkpointing", g1), ("python walk", g2)):
        for k in g0:
            d = float((g0[k] - other[k]).norm() / g0[k].norm().clamp_min(1e-30))
            assert d < 2e-6, (tag, k, d)


# ---- step and specification ----------------------------------------------------------------------------------------------------------------------------------
class _Recording:
    """Stands in for the data-parallel backend (one rank): records the slices handed to the asynchronous all-reduce."""
    active, world_size, rank = True, 1, 0

    def __init__(self):
        self.slices = []

    def broadcast_(self, t, src=0):
        pass

    def all_reduce_mean_async(self, t):
        self.slices.append((t.data_ptr(), t.numel()))


def test_control_lora_step_two_steps_against_the_restatement():
    """Two ``MI355XWanLoRAStep`` steps with ``control_latents`` against torch AdamW over the restatement's adapter parameters with the reference's clip: loss and
    pre-clip gradient norm within the existing LoRA step test's bounds at both steps; every padded adapter entry still 0; the exchange's first bucket ends at
    the buffer's end and its last starts at 0 (the patch adapter's span)."""
    import wan_control_reference as ref
    from finetrainers_amd.wan import MI355XWanControlSpecOps, MI355XWanLoRAStep
    from oracle import ltx, wan

    dev = _dev()
    omodel, gmodel = _model_pair()
    b = _batch()
    lora_before = {k: v.clone() for k, v in gmodel.lora_state_dict().items()}
    kw = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-2)
    oparams = [p for p in omodel.parameters() if p.requires_grad]
    assert len(oparams) == 32 + 2
    opt = torch.optim.AdamW(oparams, fused=False, **kw)
    spec = MI355XWanControlSpecOps()
    spec.frame_conditioning_type, spec.frame_conditioning_index = "index", 0
    par = _Recording()
    step = MI355XWanLoRAStep(gmodel, spec=spec, max_grad_norm=1.0, parallel=par, grad_bucket_blocks=1, **kw)
    args = (b["moments"].to(dev), b["text"].to(dev), b["mean"].to(dev), b["std"].to(dev), b["sigmas"].to(dev))
    for it in range(2):
        pred, target, _ = ref.spec_forward_control(omodel, b["moments"], b["control"], b["mean"], b["std"], b["text"], b["sigmas"], b["noise"], b["keep"])
        loss_ref = wan.sft_loss(pred, target, b["sigmas"])
        loss_ref.backward()
        gn_ref = float(ltx.clip_grad_norm_(oparams, 1.0))
        opt.step()
        opt.zero_grad()
        out = step.step(*args, noise=b["noise"].to(dev), control_latents=b["control"].to(dev))  # index conditioning on frame 0 = the batch's keep mask
        torch.cuda.synchronize()
        print(f"[wan-control step {it}] loss {out['loss'].item():.6f} vs {loss_ref.item():.6f}; grad_norm {out['grad_norm'].item():.5e} vs restatement {gn_ref:.5e}")
        assert abs(out["loss"].item() - loss_ref.item()) < 2e-3 * abs(loss_ref.item()) and abs(out["grad_norm"].item() - gn_ref) < 1e-2 * gn_ref
        n = step.gflat.numel()
        assert step.bucket_log[0][1] == n and step.bucket_log[-1][0] == 0 and step.bucket_log[-1] == (0, step._patch_span[1]) and len(step.bucket_log) == 3
        assert sum(hi - lo for lo, hi in step.bucket_log) == n
    after = gmodel.lora_state_dict()
    assert all(not torch.equal(after[k], lora_before[k]) for k in after), "an adapter tensor did not move"
    assert all(float(blk.lora_A.data[:, 32:].abs().max()) == 0.0 and float(blk.lora_B.data[:, :, 32:].abs().max()) == 0.0 for blk in gmodel.blocks)
    num = den = 0.0
    okeys = _lora_keys(omodel)
    for k, v in after.items():
        upd, upd_ref = v.cpu() - lora_before[k].cpu(), okeys[k].detach() - lora_before[k].cpu()
        num += float((upd - upd_ref).pow(2).sum())
        den += float(upd_ref.pow(2).sum())
    print(f"[wan-control step] adapter update vs torch.optim.AdamW on the restatement: rel L2 {math.sqrt(num / den):.3e}")
    assert step.step_count == 2


def test_specification_forward_same_bits_through_the_pack_kernel_and_through_hidden_states(parity):
    from finetrainers_amd.wan import MI355XWanControlModelSpecification

    dev = _dev()
    gmodel, b = parity["gmodel"], parity["b"]
    spec = MI355XWanControlModelSpecification(pretrained_model_name_or_path=None)
    spec._trainer_init("index", 0, False)
    res = []
    for use_pack in (True, False):
        with torch.no_grad():
            pred, target, sig = spec.forward(gmodel, {"encoder_hidden_states": b["text"].to(dev)},
                                             {"latents": b["moments"].to(dev), "control_latents": b["control"].to(dev), "latents_mean": b["mean"], "latents_std": b["std"]},
                                             b["sigmas"].to(dev), noise=b["noise"].to(dev), use_pack_kernel=use_pack)
        res.append((pred.clone(), target.clone()))
    torch.cuda.synchronize()
    assert res[0][0].shape == (2, 16, 2, 8, 12) and torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))
