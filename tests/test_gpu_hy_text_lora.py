"""HunyuanVideo LoRA with the shipped recipe's selection (eight adapters per dual-stream block: to_q / to_k / to_v / to_out.0 on the video stream and
add_q_proj / add_k_proj / add_v_proj / to_add_out on the text stream) on the GPU: the block against oracle/hunyuan.py, the C call against the Python
composition, the model, the fused step, checkpointing, fp8 storage, latent sampling and the checkpoint file."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
RECIPE = "(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|add_q_proj|add_k_proj|add_v_proj|to_add_out)"
VIDEO = ("to_q", "to_k", "to_v", "to_out.0")
TEXT = ("add_q_proj", "add_k_proj", "add_v_proj", "to_add_out")


def _dev():
    return torch.device("cuda", 0)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _rope(S, hd=128, seed=0):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(S, hd // 2, generator=g) * 6.283
    return ang.cos().repeat_interleave(2, dim=1).float().contiguous(), ang.sin().repeat_interleave(2, dim=1).float().contiguous()


def _wrap_attention(attn, names):
    """oracle.ltx.LoraLinear (peft's lora.Linear restated) around the named projections of an oracle JointAttention."""
    from oracle import ltx

    for t in names:
        if t == "to_out.0":
            attn.to_out[0] = ltx.LoraLinear(attn.to_out[0], 64, 64.0)
        else:
            setattr(attn, t, ltx.LoraLinear(getattr(attn, t), 64, 64.0))


def _block_key(k):
    for a in ("ff_context", "ff"):
        k = k.replace(f"{a}.proj_in.", f"{a}.net.0.proj.").replace(f"{a}.proj_out.", f"{a}.net.2.")
    return k


def _oracle_block(nonzero_b=True):
    from oracle import hunyuan as hy

    cfg = hy.HunyuanVideoConfig(num_attention_heads=2, attention_head_dim=128, num_layers=1, num_single_layers=0, num_refiner_layers=1, text_embed_dim=64,
                                pooled_projection_dim=32)
    torch.manual_seed(0)
    oblk = hy.DualStreamBlock(cfg)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):
            getattr(oblk.attn, n).weight.copy_(1 + 0.1 * torch.randn(128, generator=g))
    oblk = oblk.to(bf16)
    for p in oblk.parameters():
        p.requires_grad_(False)
    _wrap_attention(oblk.attn, VIDEO + TEXT)
    if nonzero_b:
        with torch.no_grad():
            for n, p in oblk.named_parameters():
                if "lora_B" in n:
                    p.normal_(0, 0.02, generator=g)
    return oblk, cfg.inner_dim


def _gpu_block(oblk, D, text_stream=True):
    from finetrainers_amd.hunyuan_video import MI355XHunyuanDualBlock

    sd = {_block_key(k): v for k, v in oblk.state_dict().items()}
    gblk = MI355XHunyuanDualBlock(dim=D, heads=2, device=_dev())
    gblk.load_diffusers_state_dict({k: v for k, v in sd.items() if "lora_" not in k})
    if text_stream:
        gblk.add_adapter(r=64, lora_alpha=64.0, text_stream=True)
    else:
        gblk.add_adapter(r=64, lora_alpha=64.0)
    with torch.no_grad():
        for i, t in enumerate(VIDEO + TEXT if text_stream else VIDEO):
            gblk.lora_A[i].copy_(sd[f"attn.{t}.lora_A.default.weight"])
            gblk.lora_B[i].copy_(sd[f"attn.{t}.lora_B.default.weight"])
    return gblk


def _block_inputs(B, T, S, D, masked):
    g = torch.Generator().manual_seed(B * 100 + S + 1)
    d = {"video": torch.randn(B, S, D, generator=g).to(bf16), "text": torch.randn(B, T, D, generator=g).to(bf16), "temb": torch.randn(B, D, generator=g).to(bf16),
         "dvid": torch.randn(B, S, D, generator=g).to(bf16), "dtxt": torch.randn(B, T, D, generator=g).to(bf16)}
    d["rope"] = _rope(S, seed=5)
    d["tmask"] = torch.ones(B, T, dtype=torch.long)
    if masked:
        d["tmask"][0, T - 3:] = 0
    d["amask"] = torch.cat([torch.ones(B, S, dtype=torch.bool), d["tmask"].bool()], dim=1).view(B, 1, 1, S + T) if masked else None
    return d


def _run_gpu_block(gblk, d, masked):
    dev = _dev()
    vg, tg = d["video"].to(dev).requires_grad_(True), d["text"].to(dev).requires_grad_(True)
    gblk.lora_A.grad = gblk.lora_B.grad = None
    ov, ot = gblk(vg, tg, d["temb"].to(dev), tuple(t.to(dev) for t in d["rope"]), text_mask=d["tmask"] if masked else None)
    torch.autograd.backward([ov, ot], [d["dvid"].to(dev), d["dtxt"].to(dev)])
    torch.cuda.synchronize()
    return ov.detach(), ot.detach(), vg.grad, tg.grad


def _block_grads(gblk, names):
    got = {}
    for i, t in enumerate(names):
        got[f"attn.{t}.lora_A.default.weight"] = gblk.lora_A.grad[i].cpu()
        got[f"attn.{t}.lora_B.default.weight"] = gblk.lora_B.grad[i].cpu()
    return got


# ---- 1. the block against the oracle -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,S,masked", [(2, 8, 40, True), (1, 16, 150, False), (1, 72, 40, False)])
def test_dual_block_with_text_adapters_matches_the_oracle(B, T, S, masked):
    """One dual-stream block with all eight adapters (r = 64, lora_B ~ N(0, 0.02), non-trivial norm weights): both outputs, both input gradients and the 16
    LoRA gradients against the oracle block.  The eight video-stream tensors keep the bounds of test_dual_stream_block_forward_backward_parity; the eight
    text-stream tensors are judged by the project's triangle (test_model_and_step_parity_small): against the same block evaluated in fp32 the kernels may be
    no further than the bf16 oracle is, with that test's margins (the noise sources are the same).  (1, 72, 40): T > S (the down-projection gradient buffer
    is sized for the longer stream) and T no multiple of 64 (ragged text rows in every LoRA GEMM).
    Figures of an MI355X run are recorded in DESIGN.md section 7-T."""
    from oracle import ltx

    oblk, D = _oracle_block()
    gblk = _gpu_block(oblk, D)
    d = _block_inputs(B, T, S, D, masked)

    def oracle_pass(blk, cast):
        for p in blk.parameters():
            p.grad = None
        vr, tr = cast(d["video"]).clone().requires_grad_(True), cast(d["text"]).clone().requires_grad_(True)
        hv, ht = blk(vr, tr, cast(d["temb"]), d["amask"], d["rope"])
        torch.autograd.backward([hv, ht], [cast(d["dvid"]), cast(d["dtxt"])])
        return hv.detach(), ht.detach(), vr.grad, tr.grad, {n: p.grad.detach().clone() for n, p in blk.named_parameters() if p.grad is not None}

    hv_ref, ht_ref, dv_ref, dt_ref, g_ref = oracle_pass(oblk, lambda t: t)
    *_, g32 = oracle_pass(copy.deepcopy(oblk).float(), lambda t: t.float())  # the same graph on the same (bf16-valued) tensors in fp32

    ov, ot, dv, dt = _run_gpu_block(gblk, d, masked)
    got = _block_grads(gblk, VIDEO + TEXT)
    assert set(got) == set(g_ref) and len(got) == 16
    e_hv, e_ht, e_dv, e_dt = _rel(ov, hv_ref), _rel(ot, ht_ref), _rel(dv, dv_ref), _rel(dt, dt_ref)
    sub = lambda grads, names: {k: v for k, v in grads.items() if any(f"attn.{t}.lora_" in k for t in names)}
    glob_v, worst_v = ltx.grads_rel_l2(sub(got, VIDEO), sub(g_ref, VIDEO))
    glob_t, worst_t = ltx.grads_rel_l2(sub(got, TEXT), sub(g_ref, TEXT))
    o32, o32_worst = ltx.grads_rel_l2(sub(g_ref, TEXT), sub(g32, TEXT))
    k32, k32_worst = ltx.grads_rel_l2(sub(got, TEXT), sub(g32, TEXT))
    print(f"[hunyuan-dual-text B={B} T={T} S={S} masked={masked}] out video {e_hv:.2e} text {e_ht:.2e} | dx video {e_dv:.2e} text {e_dt:.2e} | video LoRA grads "
          f"{glob_v:.2e} (worst {worst_v:.2e}) | text LoRA grads vs the bf16 oracle {glob_t:.2e} (worst {worst_t:.2e}); vs the fp32 evaluation: kernel k32 {k32:.2e} / "
          f"k32_worst {k32_worst:.2e}, bf16 oracle o32 {o32:.2e} / o32_worst {o32_worst:.2e}")
    assert len(sub(got, VIDEO)) == len(sub(got, TEXT)) == 8
    assert e_hv < 5e-3 and e_ht < 5e-3 and e_dv < 1e-2 and e_dt < 1e-2
    assert glob_v < 4.8e-3 and worst_v < 8e-3
    assert k32 < 1.15 * o32 + 3e-4 and k32_worst < 1.3 * o32_worst + 1e-3


# ---- 2. at initialisation -------------------------------------------------------------------------------------------------------------------------------------------
def test_text_adapters_at_initialisation_are_silent_and_learn_through_b():
    """peft's init (lora_B = 0): every adapter's contribution is zero, so the block computes what the block with video-only adapters computes; every text dA
    is exactly zero (it is a product with B), every text dB is not (it is the down-projection against the output gradient)."""
    B, T, S, masked = 2, 8, 40, True
    oblk, D = _oracle_block(nonzero_b=False)
    d = _block_inputs(B, T, S, D, masked)
    g8, g4 = _gpu_block(oblk, D, text_stream=True), _gpu_block(oblk, D, text_stream=False)
    assert tuple(g8.lora_A.shape) == (8, 64, D) and tuple(g8.lora_B.shape) == (8, D, 64) and tuple(g4.lora_A.shape) == (4, 64, D)
    assert float(g8.lora_B.detach().abs().max()) == 0.0
    out8, out4 = _run_gpu_block(g8, d, masked), _run_gpu_block(g4, d, masked)
    for (a, b), bound, n in zip(zip(out8, out4), (5e-3, 5e-3, 1e-2, 1e-2), ("video out", "text out", "d video", "d text")):
        assert _rel(a, b) < bound, n
    for i in range(4, 8):
        assert float(g8.lora_A.grad[i].abs().max()) == 0.0, TEXT[i - 4]
        assert float(g8.lora_B.grad[i].abs().max()) > 0.0, TEXT[i - 4]
    for i in range(4):
        assert float(g8.lora_A.grad[i].abs().max()) == 0.0 and float(g8.lora_B.grad[i].abs().max()) > 0.0


def test_block_add_adapter_default_is_unchanged():
    """text_stream defaults to False: shapes and RNG draws of the four-adapter block are what they were; the first four of the eight-adapter block's A are the
    same draws followed by four more."""
    from finetrainers_amd.hunyuan_video import MI355XHunyuanDualBlock

    dev = _dev()
    a, b, c = (MI355XHunyuanDualBlock(dim=256, heads=2, device=dev) for _ in range(3))
    torch.manual_seed(3)
    a.add_adapter(r=24, lora_alpha=48.0)
    torch.manual_seed(3)
    b.add_adapter(24, 48.0, False)
    torch.manual_seed(3)
    c.add_adapter(r=24, lora_alpha=48.0, text_stream=True)
    assert tuple(a.lora_A.shape) == (4, 64, 256) and tuple(a.lora_B.shape) == (4, 256, 64) and not a.text_adapters
    assert torch.equal(a.lora_A, b.lora_A) and a.lora_scale == b.lora_scale == c.lora_scale == 2.0
    assert tuple(c.lora_A.shape) == (8, 64, 256) and tuple(c.lora_B.shape) == (8, 256, 64) and c.text_adapters
    assert float(c.lora_A[:, 24:].abs().max()) == 0.0 and float(c.lora_A[:, :24].abs().min()) > 0.0 and float(c.lora_B.abs().max()) == 0.0
    assert c.lora_rank_user == 24


# ---- 3. the C call against the Python composition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,S,masked,rank,ckpt", [(2, 8, 40, True, 64, False), (1, 16, 150, False, 32, False), (2, 24, 200, True, 128, True),
                                                    (1, 72, 40, False, 64, True)])
def test_dual_block_c_call_with_text_adapters_matches_the_python_composition(B, T, S, masked, rank, ckpt):
    """``ftmi_hy_dual_forward / _backward`` with ``text_adapters = 1`` against the per-kernel composition from Python (``native = False``), which runs its text
    projections through ``ops.linear_lora_fwd / _bwd``: outputs and input gradients bit-identical, each of the 16 LoRA gradients equal up to the fp32 atomics
    of the weight-gradient GEMMs; a zero-padded rank never receives a gradient; checkpointing refills the text rows' down-projections."""
    from finetrainers_amd import ops
    from finetrainers_amd.hunyuan_video import MI355XHunyuanDualBlock

    dev = _dev()
    D = 256
    g = torch.Generator(device=dev).manual_seed(B * 1000 + S + 1)
    blk = MI355XHunyuanDualBlock(dim=D, heads=2, device=dev)
    with torch.no_grad():
        for name, buf in blk.named_buffers():
            if buf is None or name.endswith("_t") or name in ("ones", "zeros"):
                continue
            if buf.dim() == 1 and buf.numel() == 128:
                buf.copy_((1 + 0.1 * torch.randn(buf.shape, generator=g, device=dev)).to(bf16))
            elif buf.dim() == 2:
                buf.copy_((torch.randn(buf.shape, generator=g, device=dev) / buf.shape[1] ** 0.5).to(bf16))
            else:
                buf.copy_((0.02 * torch.randn(buf.shape, generator=g, device=dev)).to(bf16))
        for name in blk._TRANSPOSED:
            setattr(blk, name + "_t", ops.transpose_bf16(getattr(blk, name)))
    torch.manual_seed(2)
    blk.add_adapter(r=rank, lora_alpha=float(rank), text_stream=True)
    with torch.no_grad():
        blk.lora_B[:, :, :rank].normal_(0, 0.02, generator=g)
    blk.gradient_checkpointing = ckpt
    xv0 = torch.randn((B, S, D), generator=g, device=dev).to(bf16)
    xt0 = torch.randn((B, T, D), generator=g, device=dev).to(bf16)
    temb = torch.randn((B, D), generator=g, device=dev).to(bf16)
    dv = torch.randn((B, S, D), generator=g, device=dev).to(bf16)
    dt = torch.randn((B, T, D), generator=g, device=dev).to(bf16)
    cos, sin = _rope(S, seed=6)
    tmask = torch.ones(B, T, dtype=torch.long)
    if masked:
        tmask[0, T - 3:] = 0
    res = []
    for native in (False, True):
        blk.native = native
        blk.lora_A.grad = blk.lora_B.grad = None
        xv, xt = xv0.clone().requires_grad_(True), xt0.clone().requires_grad_(True)
        ov, ot = blk(xv, xt, temb, (cos.to(dev), sin.to(dev)), text_mask=tmask if masked else None)
        torch.autograd.backward([ov, ot], [dv, dt])
        torch.cuda.synchronize()
        res.append((ov.detach().clone(), ot.detach().clone(), xv.grad.clone(), xt.grad.clone(), blk.lora_A.grad.clone(), blk.lora_B.grad.clone()))
    r0, r1 = res
    for i, n in enumerate(("video out", "text out", "d video", "d text")):
        assert torch.equal(r0[i], r1[i]), f"{n} differs: {_rel(r1[i], r0[i]):.2e}"
    assert r1[4].shape[0] == r1[5].shape[0] == 8
    for i, n in ((4, "A"), (5, "B")):
        for j in range(8):
            assert float(r0[i][j].norm()) > 0.0
            assert float((r0[i][j] - r1[i][j]).norm() / r0[i][j].norm()) < 1e-6, (n, j)
    if blk.lora_A.shape[1] != rank:
        for r_ in res:
            assert float(r_[4][:, rank:].abs().max()) == 0.0 and float(r_[5][:, :, rank:].abs().max()) == 0.0


# ---- 4. model and step ------------------------------------------------------------------------------------------------------------------------------------------------
def _to_diffusers_key(k):
    """oracle/hunyuan.py module names -> diffusers HunyuanVideoTransformer3DModel parameter names."""
    k = k.replace("context_embedder.refiner_blocks.", "context_embedder.token_refiner.refiner_blocks.").replace(".norm_out_linear.", ".norm_out.linear.")
    if k.startswith("norm_out_linear."):
        k = "norm_out.linear." + k[len("norm_out_linear."):]
    if k.startswith("x_embedder."):
        k = "x_embedder.proj." + k[len("x_embedder."):]
    return _block_key(k)


NL, NS, GUIDANCE = 2, 2, 4.0  # (4.0 x 1000 is exact in bf16: the fp32 corner evaluates the same function, see test_model_and_step_parity_small)
KW = dict(num_attention_heads=2, attention_head_dim=128, num_layers=NL, num_single_layers=NS, num_refiner_layers=1, text_embed_dim=64, pooled_projection_dim=64)


def _oracle_model(nl=NL, ns=NS, kw=KW):
    from oracle import hunyuan as hy

    omodel = hy.build_model(hy.HunyuanVideoConfig(**dict(kw, num_layers=nl, num_single_layers=ns)), seed=0, dtype=torch.float32)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in omodel.named_parameters():
            if "norm" in n and n.endswith("weight") and p.dim() == 1:
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
    omodel = omodel.to(bf16)
    for p in omodel.parameters():
        p.requires_grad_(False)
    for blk in omodel.transformer_blocks:
        _wrap_attention(blk.attn, VIDEO + TEXT)
    for blk in omodel.single_transformer_blocks:
        _wrap_attention(blk.attn, VIDEO[:3])
    with torch.no_grad():
        for n, p in omodel.named_parameters():
            if "lora_B" in n:
                p.normal_(0, 0.02, generator=g)
    return omodel


def _gpu_model(sd, nl=NL, ns=NS, kw=KW, target=RECIPE, casting=None):
    from finetrainers_amd.hunyuan_video import HunyuanVideoTransformerConfig, MI355XHunyuanVideoTransformer3DModel

    m = MI355XHunyuanVideoTransformer3DModel(HunyuanVideoTransformerConfig(**dict(kw, num_layers=nl, num_single_layers=ns)), device=_dev())
    m.load_diffusers_state_dict(sd)
    m.add_adapter(r=64, lora_alpha=64.0, target_modules=target)
    m.load_lora_state_dict({k: v for k, v in sd.items() if "lora_" in k})
    if casting is not None:
        m.apply_layerwise_casting(real_storage=casting)
    return m


@pytest.fixture(scope="module")
def model_case():
    """The oracle model with the recipe's 280-style selection at 2 + 2 blocks, the inputs of test_model_and_step_parity_small, and the three oracle corners
    (bf16, its summation-order variant, fp32), computed once."""
    from oracle import hunyuan as hy
    from oracle import ltx

    omodel = _oracle_model()
    sd = {_to_diffusers_key(k): v for k, v in omodel.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    B, C, F_, H, W, T = 2, 16, 2, 8, 12, 8
    moments = torch.randn(B, 2 * C, F_, H, W, generator=g).to(bf16)
    moments[:, C:] = (moments[:, C:].float() * 0.3 - 2.0).to(bf16)
    eps = torch.randn(B, C, F_, H, W, generator=g).to(bf16)
    noise = torch.randn(B, C, F_, H, W, generator=g).to(bf16)
    cond = {"encoder_hidden_states": torch.randn(B, T, 64, generator=g).to(bf16), "encoder_attention_mask": torch.tensor([[1, 1, 1, 1, 1, 0, 0, 0], [1] * 8]),
            "pooled_projections": torch.randn(B, 64, generator=g).to(bf16)}
    sig = torch.tensor([0.23, 0.81])

    def corner(model, cast):
        for p_ in model.parameters():
            p_.grad = None
        c = {k: (cast(v) if v.is_floating_point() else v) for k, v in cond.items()}
        pred, target, _ = hy.spec_forward(model, cast(moments), c, sig.view(-1, 1, 1, 1, 1), cast(noise), guidance=GUIDANCE, compute_posterior=False, posterior_noise=cast(eps))
        l = (pred.float() - target.float()).pow(2)
        loss = l.mean(list(range(1, l.ndim))).mean()
        loss.backward()
        grads = {_to_diffusers_key(n).replace(".default.", "."): p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        return pred.detach(), target.detach(), loss.item(), grads

    same = lambda t: t
    pred_ref, target_ref, loss_ref, g_ref = corner(omodel, same)
    with ltx.accumulation_order_variant(128):  # the oracle's own summation-order floor on the same inputs
        _, _, _, g_alt = corner(omodel, same)
    _, _, _, g32 = corner(copy.deepcopy(omodel).float(), lambda t: t.float())
    return {"sd": sd, "moments": moments, "eps": eps, "noise": noise, "cond": cond, "sig": sig, "pred_ref": pred_ref, "target_ref": target_ref, "loss_ref": loss_ref,
            "g_ref": g_ref, "g_alt": g_alt, "g32": g32}


def _forward_backward(gmodel, case):
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoSpecOps

    dev = _dev()
    spec = MI355XHunyuanVideoSpecOps()
    for p in gmodel.lora_parameters():
        p.grad = None
    gcond = {k: v.to(dev) for k, v in case["cond"].items()}
    pred, target, _ = spec.forward(gmodel, case["moments"].to(dev), dict(gcond), case["sig"].to(dev), guidance=GUIDANCE, compute_posterior=False,
                                   posterior_noise=case["eps"].to(dev), noise=case["noise"].to(dev))
    loss = spec.loss_backward(pred, target)
    torch.cuda.synchronize()
    return pred.detach().cpu(), target.cpu(), loss.item(), {k: v.detach().cpu().clone() for k, v in gmodel.lora_grad_state_dict().items()}


def _grads_close(a, b, tol=1e-6):
    assert set(a) == set(b)
    for k in a:
        assert float((a[k].double() - b[k].double()).norm() / b[k].double().norm()) < tol, k


def test_model_gradients_of_the_recipe_selection_match_the_oracle(model_case):
    """2 dual-stream + 2 single-stream blocks under the recipe's regex: the key set is the oracle's (2 x (8 x 2 + 3 x 2) = 44 tensors; the single-stream blocks
    are what gives the last dual block's text output -- and its text adapters -- a gradient), gradients by test_model_and_step_parity_small's rule and its
    triangle; gradient checkpointing leaves the prediction bit-identical and the gradients equal up to the fp32 atomics."""
    from oracle import ltx

    case = model_case
    gmodel = _gpu_model(case["sd"])
    assert all(tuple(b.lora_A.shape) == (8, 64, 256) for b in gmodel.transformer_blocks) and all(tuple(b.lora_A.shape) == (3, 64, 256) for b in gmodel.single_transformer_blocks)
    pred, target, loss, got = _forward_backward(gmodel, case)
    g_ref, g32 = case["g_ref"], case["g32"]
    assert len(got) == 2 * (8 * NL + 3 * NS) and set(got) == set(g_ref)
    assert sum(".add_q_proj." in k or ".add_k_proj." in k or ".add_v_proj." in k or ".to_add_out." in k for k in got) == 2 * 4 * NL
    assert all(float(v.abs().max()) > 0.0 for v in got.values()), "every adapter, the last dual block's text adapters included, receives a gradient"
    floor, floor_worst = ltx.grads_rel_l2(case["g_alt"], g_ref)
    glob, worst = ltx.grads_rel_l2(got, g_ref)
    o32, o32_worst = ltx.grads_rel_l2(g_ref, g32)
    k32, k32_worst = ltx.grads_rel_l2(got, g32)
    e_pred, e_loss = _rel(pred, case["pred_ref"]), abs(loss - case["loss_ref"]) / abs(case["loss_ref"])
    print(f"[hunyuan-text-lora model {NL}+{NS}] pred {e_pred:.2e} loss rel {e_loss:.2e} | LoRA grads {glob:.2e} (worst {worst:.2e}); summation-order floor {floor:.2e} / "
          f"{floor_worst:.2e}; vs the fp32 evaluation: kernel {k32:.2e} / {k32_worst:.2e}, bf16 oracle {o32:.2e} / {o32_worst:.2e}")
    assert torch.equal(target, case["target_ref"]) and e_pred < 1e-2 and e_loss < 1e-3
    assert glob < max(2.5 * floor, 9e-3) and worst < max(2.5 * floor_worst, 1.3e-2)
    assert k32 < 1.15 * o32 + 3e-4 and k32_worst < 1.3 * o32_worst + 1e-3

    gmodel.apply_activation_checkpointing("full")
    pred_c, _, _, got_c = _forward_backward(gmodel, case)
    assert torch.equal(pred_c, pred)
    _grads_close(got_c, got)


def test_fused_step_moves_the_text_adapters_inside_its_flat_buffer(model_case):
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoSFTStep, MI355XHunyuanVideoSpecOps

    case, dev = model_case, _dev()
    gmodel = _gpu_model(case["sd"])
    gn_ref = math.sqrt(sum(float(v.double().pow(2).sum()) for v in case["g_ref"].values()))
    step = MI355XHunyuanVideoSFTStep(gmodel, MI355XHunyuanVideoSpecOps(), lr=1e-3, betas=(0.9, 0.99), guidance=GUIDANCE)
    assert step.flat.numel() == sum(p.numel() for p in gmodel.lora_parameters()) == (8 * NL + 3 * NS) * 2 * 64 * 256
    lo, hi = step.flat.data_ptr(), step.flat.data_ptr() + step.flat.numel() * 4
    for blk in gmodel.transformer_blocks:
        for p in (blk.lora_A, blk.lora_B):
            assert p.shape[0] == 8 and lo <= p[4:].data_ptr() and p[4:].data_ptr() + p[4:].numel() * 4 <= hi  # the text adapters live in the step's flat buffer
    before = [(blk.lora_A.detach().clone(), blk.lora_B.detach().clone()) for blk in gmodel.transformer_blocks]
    flat_before = step.flat.clone()
    gcond = {k: v.to(dev) for k, v in case["cond"].items()}
    out = step.step(case["moments"].to(dev), gcond, case["sig"].to(dev), compute_posterior=False, posterior_noise=case["eps"].to(dev), noise=case["noise"].to(dev))
    torch.cuda.synchronize()
    print(f"[hunyuan-text-lora step] loss {out['loss'].item():.6f} grad_norm {out['grad_norm'].item():.5e} vs oracle {gn_ref:.5e}")
    assert abs(out["loss"].item() - case["loss_ref"]) < 1e-3 * abs(case["loss_ref"]) and abs(out["grad_norm"].item() - gn_ref) < 5e-3 * gn_ref
    assert not torch.equal(step.flat, flat_before) and gmodel.transformer_blocks[0].lora_A.grad is None
    for blk, (a0, b0) in zip(gmodel.transformer_blocks, before):
        for j in range(4, 8):
            assert not torch.equal(blk.lora_A[j], a0[j]) and not torch.equal(blk.lora_B[j], b0[j]), TEXT[j - 4]


def test_real_fp8_storage_equals_the_rounded_bf16_weights_with_text_adapters(model_case):
    """apply_layerwise_casting with the text adapters on: the add_* weights come out of the shared arena (forward and transposed) like every other weight --
    identical prediction, gradients equal up to the fp32 atomics, with and without checkpointing's second up-cast."""
    case = model_case
    fake = _gpu_model(case["sd"], casting=False)
    real = _gpu_model(case["sd"], casting=True)
    assert real.transformer_blocks[0]._w8 is not None and "add_q_w" in real.transformer_blocks[0]._w8 and fake.transformer_blocks[0]._w8 is None
    pred_f, _, loss_f, got_f = _forward_backward(fake, case)
    pred_r, _, loss_r, got_r = _forward_backward(real, case)
    assert torch.equal(pred_r, pred_f) and loss_r == loss_f
    _grads_close(got_r, got_f)
    real.apply_activation_checkpointing("full")
    pred_c, _, _, got_c = _forward_backward(real, case)
    assert torch.equal(pred_c, pred_f)
    _grads_close(got_c, got_f)


# ---- 5. sampling ------------------------------------------------------------------------------------------------------------------------------------------------------
SMALL = dict(num_attention_heads=2, attention_head_dim=128, num_refiner_layers=1, text_embed_dim=64, pooled_projection_dim=64)
GRID, T_S, N_STEPS, C = (3, 8, 12), 8, 2, 16  # the smallest geometry of tests/test_gpu_hy_sampling.py's loop tests: 72 video + 8 text tokens (5 real in sample 0)


def _sample_both_ways(model, B=2, g_cfg=3.0):
    """(ftmi_hy_sample_text, model.forward + ops.hy_sample_step) on the same model: the final states."""
    import hy_sampling_reference as ref

    from finetrainers_amd import _lib, ops
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoLatentSampler, hy_flow_match_sigmas

    dev = _dev()
    g = torch.Generator().manual_seed(11)
    F_, H, W = GRID
    noise = torch.randn(B, C, F_, H, W, generator=g)
    text, pooled = torch.randn(2 * B, T_S, 64, generator=g).to(bf16).to(dev), torch.randn(2 * B, 64, generator=g).to(bf16).to(dev)  # unconditional rows first
    mask = torch.ones(2 * B, T_S, dtype=torch.bool)
    mask[B, 5:] = False
    mask = mask.to(dev)
    s = MI355XHunyuanVideoLatentSampler(model)
    geo = s.geometry(B, F_, H, W, true_cfg=True)
    S, Kc = F_ * (H // 2) * (W // 2), C * 4
    sig = hy_flow_match_sigmas(N_STEPS)
    sig_dev = sig.to(torch.float32).to(dev)
    with torch.no_grad():
        temb_silu, enc, shift, onep = s.step_tables(sig, 6.0, text, mask, pooled)
    cfg, w, keep = s.c_arguments(geo, T_S, N_STEPS, g_cfg)
    assert isinstance(cfg, _lib.HySampleTextConfig) and cfg.text_adapters == 1 and model.transformer_blocks[0].text_adapters
    x1, cols = ops.hy_sample_init(geo, noise.to(dev))
    cos, sin = (t.contiguous() for t in model._rope(*GRID))
    ops.hy_sample(cfg, w, cols, x1, temb_silu, enc, shift, onep, s.key_bias(mask, geo, T_S), cos, sin, sig_dev)
    torch.cuda.synchronize()
    del keep
    rows = 2 * B
    guidance = torch.full((rows,), 6.0, dtype=bf16, device=dev) * 1000.0
    x2, cols = ops.hy_sample_init(geo, noise.to(dev))
    for i, t in enumerate(s.timesteps(sig).tolist()):
        lat = ref.unpatchify(cols.view(rows, S, Kc), C, F_, H, W)
        with torch.no_grad():
            v = model(lat, torch.full((rows,), t, dtype=torch.float32, device=dev), text, mask, pooled, guidance=guidance)[0]
        ops.hy_sample_step(geo, ref.patchify(v).contiguous(), x2, sig_dev, i, g_cfg, cols)
    torch.cuda.synchronize()
    return x1.cpu(), x2.cpu()


def test_one_call_sampling_with_text_adapters_is_its_composition_and_sees_them():
    """Two denoising steps with an eight-adapter model (non-zero lora_B): ``ftmi_hy_sample_text`` is ``model.forward`` + ``ops.hy_sample_step`` bit for bit, and the
    result depends on the text adapters; a model whose dual blocks disagree about them is refused."""
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoLatentSampler

    omodel = _oracle_model(2, 1, SMALL)
    sd = {_to_diffusers_key(k): v for k, v in omodel.state_dict().items()}
    model = _gpu_model(sd, 2, 1, SMALL)
    bits = lambda t: t.contiguous().view(torch.int32)
    x1, x2 = _sample_both_ways(model)
    assert bool(torch.isfinite(x1).all())
    assert torch.equal(bits(x1), bits(x2)), "the one call against its composition"
    with torch.no_grad():
        for blk in model.transformer_blocks:
            blk.lora_B[4:].zero_()
    y1, y2 = _sample_both_ways(model)
    assert torch.equal(bits(y1), bits(y2))
    assert not torch.equal(bits(y1), bits(x1)), "the text adapters reach the sample"
    model.transformer_blocks[1].add_adapter(r=64, lora_alpha=64.0)  # one dual block without text adapters
    F_, H, W = GRID
    with pytest.raises(NotImplementedError, match="text-stream adapters"):
        MI355XHunyuanVideoLatentSampler(model).sample(torch.randn(1, C, F_, H, W), torch.randn(1, T_S, 64).to(bf16), None, torch.randn(1, 64).to(bf16), num_inference_steps=1)


# ---- 6. the checkpoint file ------------------------------------------------------------------------------------------------------------------------------------------
def test_recipe_checkpoint_round_trip_through_the_specification(tmp_path):
    """``_save_lora_weights`` writes 2 x (8 nl + 3 ns) ``transformer.``-prefixed tensors and the recipe's ``target_modules`` string; the file loads back exactly;
    a file and a model that disagree about the text adapters raise in both directions."""
    from safetensors import safe_open

    from finetrainers_amd import wire
    from finetrainers_amd.hunyuan_video import HunyuanVideoTransformerConfig, MI355XHunyuanVideoModelSpecification, MI355XHunyuanVideoTransformer3DModel

    nl, ns, r = 2, 3, 24
    cfg = HunyuanVideoTransformerConfig(**dict(KW, num_layers=nl, num_single_layers=ns))
    new = lambda: MI355XHunyuanVideoTransformer3DModel(cfg, device=_dev())
    model = new()
    model.add_adapter(r=r, lora_alpha=48.0, target_modules=RECIPE)
    g = torch.Generator(device=_dev()).manual_seed(5)
    with torch.no_grad():
        for blk in list(model.transformer_blocks) + list(model.single_transformer_blocks):
            blk.lora_B[:, :, :r].normal_(0, 0.02, generator=g)
    sd = model.lora_state_dict()
    assert len(sd) == 2 * (8 * nl + 3 * ns) and len(model.lora_parameters()) == 2 * (nl + ns)
    assert tuple(sd["transformer_blocks.1.attn.to_add_out.lora_A.weight"].shape) == (r, 256) and tuple(sd["transformer_blocks.1.attn.add_k_proj.lora_B.weight"].shape) == (256, r)
    assert sd["transformer_blocks.0.attn.add_q_proj.lora_A.weight"].data_ptr() == model.transformer_blocks[0].lora_A[4].data_ptr()  # views, not copies
    spec = MI355XHunyuanVideoModelSpecification(pretrained_model_name_or_path=None)
    out = tmp_path / "ckpt"
    spec._save_lora_weights(str(out), sd, None, model.lora_config_metadata())
    with safe_open(str(out / "pytorch_lora_weights.safetensors"), framework="pt") as f:
        keys = list(f.keys())
    assert len(keys) == 2 * (8 * nl + 3 * ns) and all(k.startswith("transformer.") for k in keys)
    assert "transformer.transformer_blocks.0.attn.add_v_proj.lora_B.weight" in keys
    tensors, lcfg = wire.load_lora_weights(str(out))
    assert lcfg["target_modules"] == RECIPE and lcfg["r"] == r and lcfg["lora_alpha"] == 48.0
    assert set(tensors) == set(sd)

    again = new()
    again.add_adapter(r=r, lora_alpha=48.0, target_modules=lcfg["target_modules"])
    again.load_lora_state_dict(tensors)
    back = again.lora_state_dict()
    for k, v in sd.items():
        assert torch.equal(back[k].cpu(), v.cpu()), k
    for a, b in zip(again.transformer_blocks, model.transformer_blocks):
        assert torch.equal(a.lora_A, b.lora_A) and torch.equal(a.lora_B, b.lora_B)  # the zero padding included

    video_only = new()
    video_only.add_adapter(r=r, lora_alpha=48.0)
    assert len(video_only.lora_state_dict()) == 2 * (4 * nl + 3 * ns)
    # (the default selection's metadata names the reference's default regex)
    assert "to_out.0)" in video_only.lora_config_metadata()["lora_config"] and "add_q_proj" not in video_only.lora_config_metadata()["lora_config"]
    with pytest.raises(KeyError, match="no adapter for"):
        video_only.load_lora_state_dict(tensors)  # a file with text keys into a model without text adapters
    with pytest.raises(KeyError, match="lacks transformer_blocks.0.attn.add_q_proj"):
        again.load_lora_state_dict({k: v.cpu() for k, v in video_only.lora_state_dict().items()})  # a file that lacks keys the model has
    for k, v in sd.items():
        assert torch.equal(again.lora_state_dict()[k].cpu(), v.cpu()), "a refused load changes nothing"
