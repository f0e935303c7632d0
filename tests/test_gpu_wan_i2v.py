"""Wan image-to-video LoRA on the GPU: the second-context attention kernels (``ftmi_attn_ctx2_fwd / _dq``) against fp64, their tail and saturation
behaviour, the I2V block's exact degenerations to the T2V LoRA block, block / model / step parity against tests/wan_i2v_reference.py (oracle.wan extended
with the image embedder and the image branch of attn2), the C call against the Python composition and recomputation against the kept activations."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
SMALL, REAL, BIG = (256, 2, 512), (1536, 12, 8960), (5120, 40, 13824)  # (D, H, F); BIG = Wan2.1-I2V-14B
TI = 257


def _dev():
    return torch.device("cuda", 0)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ---- 1, 2: the kernels ----------------------------------------------------------------------------------------------------------------------------------
def _ctx2_case(B, H, Sq, Sk, seed, alloc=None):
    """bf16 tensors in the block's layouts: q, o_t, dO, dq_t inside [B, Sq, H 128] rows, k_i | v_i the two halves of a [B, alloc, 2 H 128] row."""
    g = torch.Generator().manual_seed(seed)
    D = H * 128
    heads = lambda t, n: t.view(B, n, H, 128).permute(0, 2, 1, 3)
    q, o_t, do, dq_t = (torch.randn(B, Sq, D, generator=g).to(bf16) for _ in range(4))
    kv = torch.randn(B, alloc or Sk, 2 * D, generator=g).to(bf16)
    return dict(q=heads(q, Sq), o_t=heads(o_t, Sq), do=heads(do, Sq), dq_t=heads(dq_t, Sq), kv=kv, Sk=Sk, H=H)


def _kv_views(kv, Sk, H):
    B, D = kv.shape[0], kv.shape[2] // 2
    heads = lambda t: t.unflatten(2, (H, 128)).permute(0, 2, 1, 3)
    return heads(kv[:, :Sk, :D]), heads(kv[:, :Sk, D:])


def _run_ctx2(c, kv=None):
    from finetrainers_amd import ops

    dev = _dev()
    k, v = _kv_views((c["kv"] if kv is None else kv).to(dev), c["Sk"], c["H"])
    # .to(dev) of a permuted view keeps its strides: q / o_t / dO / dq_t stay rows of a [B, Sq, D] tensor
    q, o_t, do, dq_t = (c[n].to(dev) for n in ("q", "o_t", "do", "dq_t"))
    assert q.stride(1) == 128 and q.stride(2) == c["H"] * 128 and (c["Sk"] == 1 or k.stride(2) == 2 * c["H"] * 128)
    o, lse = ops.attn_ctx2_fwd(q, k, v, o_t)
    dq = ops.attn_ctx2_dq(q, k, v, lse, do, dq_t)
    torch.cuda.synchronize()
    return o.cpu(), dq.cpu(), lse.cpu()


def _check_ctx2(c, tag):
    """Relative L2 from fp64 of o and dq at most 2 x that of the bf16-storage torch graph (the project's kernel-vs-oracle margin).  lse: the kernel sums the
    bf16-rounded probabilities that feed P.V (relative error of the sum <= 2^-9), so |lse - fp64| <= 2^-9 log2(e) = 2.8e-3, plus fp32 noise on the scores
    (<= 1e-5 |lse|); 4e-3 + 1e-5 |lse| is asserted."""
    import wan_i2v_reference as ref

    k, v = _kv_views(c["kv"], c["Sk"], c["H"])
    args = (c["q"], k, v, c["o_t"], c["do"], c["dq_t"])
    o64, dq64, lse64 = ref.ctx2_fp64(*args)
    ob, dqb, _ = ref.ctx2_bf16_storage(*args)
    o, dq, lse = _run_ctx2(c)
    assert torch.isfinite(o.float()).all() and torch.isfinite(dq.float()).all() and torch.isfinite(lse).all()
    for name, got, yard, want in (("o", o, ob, o64), ("dq", dq, dqb, dq64)):
        e, y = _rel(got, want), _rel(yard, want)
        print(f"[ctx2 {tag}] {name}: kernel vs fp64 {e:.3e}, bf16-storage graph vs fp64 {y:.3e}, ratio {e / max(y, 1e-300):.2f}")
        assert e <= 2.0 * y, (name, e, y)
    d = (lse.double() - lse64).abs()
    print(f"[ctx2 {tag}] lse: max |kernel - fp64| {d.max().item():.2e}")
    assert (d <= 4e-3 + 1e-5 * lse64.abs()).all()
    return o, dq, lse


@pytest.mark.parametrize("Sk", [1, 64, 256, 257, 320])
@pytest.mark.parametrize("B,H,Sq", [(2, 2, 48), (1, 12, 200), (2, 2, 320)])
def test_ctx2_kernels_against_fp64(B, H, Sq, Sk):
    _check_ctx2(_ctx2_case(B, H, Sq, Sk, seed=B * 100000 + Sq * 1000 + Sk), f"B={B} H={H} Sq={Sq} TI={Sk}")


def test_ctx2_tail_key_and_saturated_rows():
    """TI = 257 (four full tiles and a tail of one key).  Query row 0 of every head: all real logits below -100; row 1: dominated by the single tail key.
    o, lse and dq finite and within the bounds of the test above; NaN in the allocation behind key 257 of k_i / v_i changes no bit."""
    import wan_i2v_reference as ref

    B, H, Sq = 1, 2, 48
    c = _ctx2_case(B, H, Sq, TI, seed=5, alloc=320)
    g = torch.Generator().manual_seed(6)
    u = torch.full((128,), 128 ** -0.5)
    w = torch.zeros(128)
    w[0], w[1] = 2 ** -0.5, -(2 ** -0.5)  # unit, orthogonal to u
    kv = c["kv"].float().view(B, 320, 2, H, 128)
    kv[:, :, 0] = 12.0 * u + 0.3 * torch.randn(B, 320, H, 128, generator=g)
    kv[:, TI - 1, 0] += 6.0 * w
    c["kv"] = kv.view(B, 320, 2 * H * 128).to(bf16)
    q = c["q"].float().clone()
    q[:, :, 0] = -110.0 * u + 0.1 * torch.randn(B, H, 128, generator=g)
    q[:, :, 1] = 40.0 * w
    c["q"] = q.permute(0, 2, 1, 3).contiguous().to(bf16).permute(0, 2, 1, 3)
    k, _ = _kv_views(c["kv"], TI, H)
    logits = (c["q"].double() @ k.double().transpose(-1, -2)) / 128 ** 0.5
    assert logits[:, :, 0].max() < -100.0
    assert (logits[:, :, 1, TI - 1] - logits[:, :, 1, :TI - 1].max(-1).values).min() > 10.0
    o, dq, lse = _check_ctx2(c, "saturated rows + tail key")
    poisoned = c["kv"].clone()
    poisoned[:, TI:] = float("nan")
    o2, dq2, lse2 = _run_ctx2(c, kv=poisoned)
    assert torch.equal(o, o2) and torch.equal(dq, dq2) and torch.equal(lse, lse2)


# ---- blocks ---------------------------------------------------------------------------------------------------------------------------------------------
def _rope_tables(S, hd, seed=0):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(S, hd // 2, generator=g, dtype=torch.float64) * 6.283
    return (torch.cos(ang).float(), torch.sin(ang).float()), torch.polar(torch.ones_like(ang), ang).view(1, 1, S, hd // 2)


def _fix(k):
    return k.replace("ffn.proj_in.", "ffn.net.0.proj.").replace("ffn.proj_out.", "ffn.net.2.")


def _lora_keys(m):
    return {n.replace(".default.", "."): p for n, p in m.named_parameters() if "lora_" in n}


def _wrap(attn, rank, alpha, g, b_std=0.02):
    from oracle import ltx

    for t in ("to_q", "to_k", "to_v"):
        setattr(attn, t, ltx.LoraLinear(getattr(attn, t), rank, alpha))
    attn.to_out[0] = ltx.LoraLinear(attn.to_out[0], rank, alpha)
    with torch.no_grad():
        for n, p in attn.named_parameters():
            if "lora_B" in n:
                p.normal_(0, b_std, generator=g)


def _perturb(module, g):
    with torch.no_grad():
        for n, p in module.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))


def _block_pair(geom, rank, oracle=True, seed=0):
    """(reference I2V block with LoraLinear on the eight projections, or None; MI355XWanBlock(added_kv_proj_dim) with the same weights and adapters)."""
    import wan_i2v_reference as ref
    from finetrainers_amd.wan import LORA_TARGETS, MI355XWanBlock

    D, heads, ffn = geom
    cfg = ref.WanI2VConfig(num_attention_heads=heads, attention_head_dim=128, ffn_dim=ffn, num_layers=1, text_dim=64)
    torch.manual_seed(seed)
    oblk = ref.WanI2VTransformerBlock(cfg)
    g = torch.Generator().manual_seed(7)
    _perturb(oblk, g)
    oblk = oblk.to(bf16)
    gblk = MI355XWanBlock(dim=D, heads=heads, ffn_dim=ffn, eps=cfg.eps, device=_dev(), added_kv_proj_dim=D)
    gblk.load_diffusers_state_dict({_fix(k): v for k, v in oblk.state_dict().items()})
    for p in oblk.parameters():
        p.requires_grad_(False)
    for attn in (oblk.attn1, oblk.attn2):
        _wrap(attn, rank, float(rank), g)
    gblk.add_adapter(rank, float(rank))
    keys = _lora_keys(oblk)
    with torch.no_grad():
        for j, n in enumerate(LORA_TARGETS):
            gblk.lora_A.data[j, :rank].copy_(keys[f"{n}.lora_A.weight"])
            gblk.lora_B.data[j, :, :rank].copy_(keys[f"{n}.lora_B.weight"])
    return (oblk if oracle else None), gblk


def _t2v_twin(gblk):
    """The T2V LoRA block with gblk's base weights and adapters."""
    from finetrainers_amd.wan import MI355XWanBlock

    t = MI355XWanBlock(dim=gblk.dim, heads=gblk.heads, ffn_dim=gblk.ffn_dim, eps=gblk.eps, device=_dev())
    t.flat.data.copy_(gblk.flat.data)
    t.mark_updated()
    t.add_adapter(gblk.lora_rank_user, gblk.lora_scale * gblk.lora_rank_user)
    t.lora_A.data.copy_(gblk.lora_A.data)
    t.lora_B.data.copy_(gblk.lora_B.data)
    return t


def _inputs(B, S, T, D, seed, ti=TI):
    g = torch.Generator().manual_seed(seed)
    x, enc = torch.randn(B, S, D, generator=g).to(bf16), torch.randn(B, T, D, generator=g).to(bf16)
    temb, dout = (0.5 * torch.randn(B, 6, D, generator=g)).to(bf16), torch.randn(B, S, D, generator=g).to(bf16)
    return x, enc, temb, dout, torch.randn(B, ti, D, generator=g).to(bf16)


def _run_gpu(gblk, x, enc, temb, dout, rope, img=None):
    dev = _dev()
    xg, eg = x.to(dev).requires_grad_(True), enc.to(dev).requires_grad_(True)
    gblk.lora_A.grad = gblk.lora_B.grad = None
    extra = () if img is None else (img.to(dev),)
    out = gblk(xg, eg, temb.to(dev), (rope[0].to(dev), rope[1].to(dev)), *extra)
    out.backward(dout.to(dev))
    torch.cuda.synchronize()
    return out.detach().clone(), xg.grad.clone(), eg.grad.clone(), gblk.lora_A.grad.clone(), gblk.lora_B.grad.clone()


def _same(r0, r1, tag):
    """out, dx, d text bit-equal; the 16 adapter gradients within the order of their fp32 atomics (2e-6, the T2V tests' bound)."""
    for i, n in enumerate(("output", "dx", "d text")):
        assert torch.equal(r0[i], r1[i]), f"{tag}: {n} differs: {_rel(r1[i], r0[i]):.2e}"
    for i, n in ((3, "lora_A"), (4, "lora_B")):
        for j in range(8):
            d = float((r0[i][j] - r1[i][j]).norm() / r0[i][j].norm().clamp_min(1e-30))
            assert d < 2e-6, (tag, n, j, d)


CASES = [(SMALL, 2, 48, 16), (REAL, 1, 200, 64)]


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("geom,B,S,T", CASES)
def test_i2v_block_exact_degenerations(geom, B, S, T, native):
    """TI = 0: the bits of the T2V LoRA block.  add_v_proj = 0 with TI = 257: o_i = 0 and dP_i = 0, so dq_i = 0 -- again the T2V block's out, dx, d text
    bits (adapter gradients to the order of their atomics).  Through the C call and through the Python composition."""
    _, gblk = _block_pair(geom, 32, oracle=False)
    t2v = _t2v_twin(gblk)
    gblk.native = t2v.native = native
    x, enc, temb, dout, img = _inputs(B, S, T, geom[0], seed=S)
    rope, _ = _rope_tables(S, 128, seed=4)
    want = _run_gpu(t2v, x, enc, temb, dout, rope)
    _same(want, _run_gpu(gblk, x, enc, temb, dout, rope, img[:, :0]), "TI = 0")
    live = _run_gpu(gblk, x, enc, temb, dout, rope, img)
    assert not torch.equal(live[0], want[0]), "the image branch contributes nothing"
    gblk.img_param("attn2.add_v_proj.weight").zero_()
    gblk.img_param("attn2.add_v_proj.bias").zero_()
    _same(want, _run_gpu(gblk, x, enc, temb, dout, rope, img), "add_v_proj = 0")


@pytest.mark.parametrize("rank", [32, 64])
@pytest.mark.parametrize("geom,B,S,T", CASES + [(BIG, 1, 136, 16)])
def test_i2v_block_c_call_python_composition_and_recomputation(geom, B, S, T, rank):
    """``ftmi_wan_lora_ffn_block_*`` (TI > 0, ffn = 0) against the per-kernel composition from Python, and the C call with gradient checkpointing (``out = NULL`` refills the
    saved buffer inside the backward) against the kept activations: same bits, adapter gradients to the order of their atomics."""
    _, gblk = _block_pair(geom, rank, oracle=False)
    x, enc, temb, dout, img = _inputs(B, S, T, geom[0], seed=S + 7)
    rope, _ = _rope_tables(S, 128, seed=4)
    res = []
    for native, ckpt in ((False, False), (True, False), (True, True), (False, True)):
        gblk.native, gblk.gradient_checkpointing = native, ckpt
        res.append(_run_gpu(gblk, x, enc, temb, dout, rope, img))
    for r, tag in zip(res[1:], ("C call", "C call, recomputed", "python, recomputed")):
        _same(res[0], r, tag)


def _oracle_run(blk, cast, x, enc, temb, dout, freqs, img):
    for p in blk.parameters():
        p.grad = None
    xr, er = (t.to(cast).clone().requires_grad_(True) for t in (x, enc))
    out = blk(xr, er, temb.to(cast), freqs, img.to(cast))
    out.backward(dout.to(cast))
    return out.detach(), xr.grad, er.grad, {k: p.grad.detach().clone() for k, p in _lora_keys(blk).items()}


@pytest.mark.parametrize("rank", [32, 64])
@pytest.mark.parametrize("geom,B,S,T", CASES + [(BIG, 1, 136, 16)])
def test_i2v_block_parity(geom, B, S, T, rank):
    """Forward + backward against the bf16 CPU reference and its fp32 evaluation, with test_lora_block_parity's bounds (out 5e-3, dx 1e-2, the 16 adapter
    gradients in the floor form).  d text has no bound there; it goes through the same chain of roundings as dx and gets dx's bound."""
    from finetrainers_amd.wan import LORA_TARGETS
    from oracle import ltx

    oblk, gblk = _block_pair(geom, rank)
    x, enc, temb, dout, img = _inputs(B, S, T, geom[0], seed=B * 1000 + S)
    rope, freqs = _rope_tables(S, 128, seed=3)
    o_ref, dx_ref, de_ref, g_ref = _oracle_run(oblk, bf16, x, enc, temb, dout, freqs, img)
    o32, dx32, de32, g32 = _oracle_run(oblk.float(), torch.float32, x, enc, temb, dout, freqs, img)
    floor, floor_worst = ltx.grads_rel_l2(g_ref, g32)
    out, dx, de, ga, gb = _run_gpu(gblk, x, enc, temb, dout, rope, img)
    got = {}
    for j, n in enumerate(LORA_TARGETS):
        got[f"{n}.lora_A.weight"], got[f"{n}.lora_B.weight"] = ga[j, :rank].cpu(), gb[j, :, :rank].cpu()
    assert set(got) == set(g_ref) and len(got) == 16
    glob, worst = ltx.grads_rel_l2(got, g_ref)
    glob32, worst32 = ltx.grads_rel_l2(got, g32)
    e_o, e_dx, e_de = _rel(out, o_ref), _rel(dx, dx_ref), _rel(de, de_ref)
    print(f"[wan-i2v block D={geom[0]} B={B} S={S} T={T} r={rank}] out {e_o:.2e} (ref bf16 vs fp32 {_rel(o_ref, o32):.2e}) | dx {e_dx:.2e} ({_rel(dx_ref, dx32):.2e}) "
          f"d text {e_de:.2e} ({_rel(de_ref, de32):.2e}) | adapter grads vs bf16 ref {glob:.2e} (worst {worst:.2e}), vs fp32 ref {glob32:.2e} (worst {worst32:.2e}); "
          f"bf16 ref vs fp32 ref {floor:.2e} (worst {floor_worst:.2e})")
    assert e_o < 5e-3 and e_dx < 1e-2 and e_de < 1e-2
    assert glob < 2.0 * floor + 2e-3 and worst < 2.0 * floor_worst + 5e-3
    assert glob32 < 1.5 * floor + 1e-3 and worst32 < 1.5 * floor_worst + 2e-3


# ---- 5: model and step ----------------------------------------------------------------------------------------------------------------------------------
KW = dict(num_attention_heads=2, attention_head_dim=128, ffn_dim=512, text_dim=64, image_dim=128)


def _model_pair(layers=2, rank=32):
    import wan_i2v_reference as ref
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig

    torch.manual_seed(0)
    omodel = ref.WanI2VTransformer3DModel(ref.WanI2VConfig(num_layers=layers, **KW))
    g = torch.Generator().manual_seed(7)
    _perturb(omodel, g)
    omodel = omodel.to(bf16)
    gmodel = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, in_channels=36, **KW), device=_dev())
    gmodel.load_diffusers_state_dict({_fix(k): v for k, v in omodel.state_dict().items()})
    for p in omodel.parameters():
        p.requires_grad_(False)
    for blk in omodel.blocks:
        for attn in (blk.attn1, blk.attn2):
            _wrap(attn, rank, float(rank), g)
    gmodel.add_adapter(rank, float(rank))
    gmodel.load_lora_state_dict({k: v.detach() for k, v in _lora_keys(omodel).items()})
    return omodel, gmodel


@functools.lru_cache(maxsize=None)
def _batch():
    g = torch.Generator().manual_seed(11)
    B, C, F_, H, W = 2, 16, 2, 8, 12  # 2 x 4 x 6 = 48 tokens
    mom = lambda: torch.cat([torch.randn(B, C, F_, H, W, generator=g), 0.3 * torch.randn(B, C, F_, H, W, generator=g) - 2.0], dim=1).to(bf16)
    return dict(moments=mom(), cond=mom(), mask=(torch.rand(B, 4, F_, H, W, generator=g) < 0.3).to(bf16), text=torch.randn(B, 16, 64, generator=g).to(bf16),
                image=torch.randn(B, TI, 128, generator=g).to(bf16), eps=torch.randn(B, C, F_, H, W, generator=g).to(bf16),
                noise=torch.randn(B, C, F_, H, W, generator=g).to(bf16), sigmas=torch.tensor([0.23, 0.81]), mean=0.1 * torch.randn(C, generator=g),
                std=1.0 + 0.2 * torch.rand(C, generator=g))


def _oracle_model_run(model, cast, b):
    import wan_i2v_reference as ref
    from oracle import wan

    for p in model.parameters():
        p.grad = None
    c = lambda t: t.to(cast)
    pred, target, _ = ref.spec_forward_i2v(model, c(b["moments"]), b["mean"], b["std"], c(b["text"]), b["sigmas"].view(-1, 1, 1, 1, 1), c(b["eps"]), c(b["noise"]),
                                           c(b["cond"]), c(b["mask"]), c(b["image"]))
    loss = wan.sft_loss(pred, target, b["sigmas"])
    loss.backward()
    return loss, pred.detach(), {k: p.grad.detach().clone() for k, p in _lora_keys(model).items()}


def _gpu_kwargs(b):
    d = lambda t: t.to(_dev())
    return dict(posterior_noise=d(b["eps"]), noise=d(b["noise"]), latent_condition=d(b["cond"]), latent_condition_mask=d(b["mask"]),
                encoder_hidden_states_image=d(b["image"]))


def test_i2v_model_parity():
    """A 2-block I2V model (36 input channels, image embedder, 257 image tokens): prediction, loss and the 32 adapter gradients against the reference, with
    the bounds of the T2V model test."""
    from finetrainers_amd.wan import MI355XWanSpecOps
    from oracle import ltx

    omodel, gmodel = _model_pair()
    b = _batch()
    loss_ref, pred_ref, g_ref = _oracle_model_run(omodel, bf16, b)
    _, pred32, g32 = _oracle_model_run(copy.deepcopy(omodel).float(), torch.float32, b)
    floor, floor_worst = ltx.grads_rel_l2(g_ref, g32)
    dev, spec = _dev(), MI355XWanSpecOps()
    pred, target, _ = spec.forward(gmodel, b["moments"].to(dev), b["text"].to(dev), b["sigmas"].to(dev), b["mean"].to(dev), b["std"].to(dev), **_gpu_kwargs(b))
    loss = spec.loss_backward(pred, target).item()
    torch.cuda.synchronize()
    got = {k: v.detach().cpu() for k, v in gmodel.lora_grad_state_dict().items()}
    assert set(got) == set(g_ref) and len(got) == 32
    glob, worst = ltx.grads_rel_l2(got, g_ref)
    glob32, worst32 = ltx.grads_rel_l2(got, g32)
    e_pred, e_loss = _rel(pred.detach(), pred_ref), abs(loss - loss_ref.item()) / abs(loss_ref.item())
    print(f"[wan-i2v model] pred {e_pred:.2e} (ref bf16 vs fp32 {_rel(pred_ref, pred32):.2e}) loss rel {e_loss:.2e} | adapter grads vs bf16 ref {glob:.2e} "
          f"(worst {worst:.2e}), vs fp32 ref {glob32:.2e} (worst {worst32:.2e}); floor {floor:.2e} (worst {floor_worst:.2e})")
    assert e_pred < 2e-2 and e_loss < 3e-3
    assert glob < 2.0 * floor + 2e-3 and worst < 2.0 * floor_worst + 5e-3
    assert glob32 < 1.5 * floor + 1e-3 and worst32 < 1.5 * floor_worst + 2e-3


def _two_steps(ckpt, with_reference=False):
    """Two ``MI355XWanLoRAStep`` steps on a fresh model pair -> dict(losses, grad norms, prediction before and after, adapters before and after, model);
    ``with_reference``: the same two steps with torch AdamW on the bf16 reference and on its fp32 evaluation (losses, norms, adapters after)."""
    from finetrainers_amd.wan import MI355XWanLoRAStep, MI355XWanSpecOps
    from oracle import ltx

    dev, b = _dev(), _batch()
    kw = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-2)
    args = tuple(b[n].to(dev) for n in ("moments", "text", "mean", "std", "sigmas"))
    omodel, gmodel = _model_pair()
    if ckpt:
        gmodel.apply_activation_checkpointing()
        assert all(blk.gradient_checkpointing for blk in gmodel.blocks)

    def predict():
        with torch.no_grad():
            return MI355XWanSpecOps().forward(gmodel, args[0], args[1], args[4], args[2], args[3], **_gpu_kwargs(b))[0].clone()

    r = dict(before={k: v.clone().cpu() for k, v in gmodel.lora_state_dict().items()}, pred0=predict(), model=gmodel, losses=[], norms=[])
    r["step"] = step = MI355XWanLoRAStep(gmodel, max_grad_norm=1.0, **kw)
    for _ in range(2):
        out = step.step(*args, **_gpu_kwargs(b))
        torch.cuda.synchronize()
        r["losses"].append(out["loss"].item())
        r["norms"].append(out["grad_norm"].item())
    r["after"] = {k: v.clone().cpu() for k, v in gmodel.lora_state_dict().items()}
    r["pred2"] = predict()
    if with_reference:
        for tag, model, cast in (("ref", omodel, bf16), ("ref32", copy.deepcopy(omodel).float(), torch.float32)):
            oparams = [p for p in model.parameters() if p.requires_grad]
            assert len(oparams) == 32
            opt = torch.optim.AdamW(oparams, fused=False, **kw)
            losses, norms = [], []
            for _ in range(2):
                loss, _, _ = _oracle_model_run(model, cast, b)
                losses.append(loss.item())
                norms.append(float(ltx.clip_grad_norm_(oparams, 1.0)))
                opt.step()
            r[tag] = dict(losses=losses, norms=norms, after={k: p.detach().clone() for k, p in _lora_keys(model).items()})
    return r


def _update_distance(after, after_ref, before):
    num = den = 0.0
    for k, v in after.items():
        upd, upd_ref = v.float() - before[k], after_ref[k].float() - before[k]
        num += float((upd - upd_ref).pow(2).sum())
        den += float(upd_ref.pow(2).sum())
    return (num / den) ** 0.5


def test_i2v_lora_step_with_and_without_checkpointing():
    """Two ``MI355XWanLoRAStep`` steps on the I2V model.

    Against torch AdamW on the reference's adapters: loss within 2e-3 and pre-clip gradient norm within 1e-2 at both steps (the T2V step test's bounds), and
    the adapters' UPDATE after the two steps within 2 x the distance between the reference's own bf16 and fp32 evaluations taken through the same two
    AdamW steps (first-step Adam is sign-like, so entries with near-zero gradients flip between any two evaluations: that distance is the yardstick, 2 x the
    project's kernel-vs-oracle margin).

    Checkpointing on against off: the prediction before the steps and the first loss have the same bits.  The adapter gradients are sums of fp32 atomics
    whose order is not fixed, so what follows an UPDATE (second loss, prediction after the steps) is reproducible only as far as a plain rerun of the same
    configuration is: it must be bit-equal under checkpointing unless the rerun without checkpointing differs from the first run as well (deviation from
    "same bits after two steps"; the three spreads are printed and recorded in profiles/wan_i2v_ab.txt), and the second loss stays within 1e-5 either way.
    From IDENTICAL adapter state after the two steps, a forward + loss with checkpointing on and off has the same bits and the 32 adapter gradients of
    its backward agree to 2e-6, the bound of test_activation_checkpointing_same_loss_and_prediction_bits."""
    from finetrainers_amd.wan import MI355XWanSpecOps

    a, c, rerun = _two_steps(False, with_reference=True), _two_steps(True), _two_steps(False)
    for it in range(2):
        print(f"[wan-i2v step {it}] loss {a['losses'][it]:.6f} vs {a['ref']['losses'][it]:.6f}; grad_norm {a['norms'][it]:.5e} vs {a['ref']['norms'][it]:.5e}")
        assert abs(a["losses"][it] - a["ref"]["losses"][it]) < 2e-3 * abs(a["ref"]["losses"][it])
        assert abs(a["norms"][it] - a["ref"]["norms"][it]) < 1e-2 * a["ref"]["norms"][it]
    assert all(not torch.equal(a["after"][k], a["before"][k]) for k in a["after"]), "an adapter tensor did not move"
    d_gpu = _update_distance(a["after"], a["ref"]["after"], a["before"])
    d_floor = _update_distance(a["ref32"]["after"], a["ref"]["after"], a["before"])
    print(f"[wan-i2v step] adapter update after two steps vs torch.optim.AdamW on the bf16 reference: rel L2 {d_gpu:.3e}; fp32 reference vs bf16 reference {d_floor:.3e}")
    assert d_gpu <= 2.0 * d_floor, (d_gpu, d_floor)
    # checkpointing: bits
    assert torch.equal(a["pred0"], c["pred0"]) and a["losses"][0] == c["losses"][0], "prediction / first loss bits differ under checkpointing"
    same = lambda x, y: x["losses"][1] == y["losses"][1] and torch.equal(x["pred2"], y["pred2"])
    for tag, other in (("checkpointing", c), ("plain rerun", rerun)):
        print(f"[wan-i2v step] {tag} vs first run: second loss {other['losses'][1]!r} vs {a['losses'][1]!r}, prediction after two steps rel {_rel(other['pred2'], a['pred2']):.2e}, "
              f"adapters rel {_update_distance(other['after'], a['after'], a['before']):.2e}")
    assert same(a, c) or not same(a, rerun), "checkpointing changed bits that a plain rerun reproduces"
    # where the bits do differ, the distance stays bounded: the gradients agree to 2e-6 (below), first-step Adam is insensitive to a relative change of
    # its gradient, so the second loss moves only through a few bf16 roundings downstream of adapters that agree to ~1e-7 -- 1e-5, 200 x below the
    # bound on the loss against the reference
    for other in (c, rerun):
        assert abs(other["losses"][1] - a["losses"][1]) <= 1e-5 * abs(a["losses"][1])
    # identical adapter state: checkpointing off and on give the same forward and loss bits
    c["model"].load_lora_state_dict({k: v.to(_dev()) for k, v in a["after"].items()})
    dev, b, spec = _dev(), _batch(), MI355XWanSpecOps()
    res = []
    for r in (a, c):
        r["step"].gflat.zero_()  # the backward below adds into the step object's gradient views
        pred, target, _ = spec.forward(r["model"], b["moments"].to(dev), b["text"].to(dev), b["sigmas"].to(dev), b["mean"].to(dev), b["std"].to(dev), **_gpu_kwargs(b))
        loss = spec.loss_backward(pred, target).item()
        torch.cuda.synchronize()
        res.append((loss, pred.detach().clone(), {k: v.detach().clone() for k, v in r["model"].lora_grad_state_dict().items()}))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]), "same adapters, checkpointing on / off: loss or prediction bits differ"
    worst = max(float((res[0][2][k] - res[1][2][k]).norm() / res[0][2][k].norm().clamp_min(1e-30)) for k in res[0][2])
    print(f"[wan-i2v step] same adapters, checkpointing on vs off: 32 adapter gradients, worst rel {worst:.2e}")
    assert len(res[0][2]) == 32 and worst < 2e-6  # recomputed activations: the same operands, summed by fp32 atomics in another order (the T2V test's bound)
