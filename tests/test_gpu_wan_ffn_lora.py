"""Wan LoRA with adapters on the feed-forward projections as well (--target_modules "blocks.*(to_q|to_k|to_v|to_out.0|ffn.net.0.proj|ffn.net.2)": ten
adapters per block) on the GPU: the ten-adapter block with B = 0 on the feed-forward against the eight-adapter block's bits (both through the one C entry,
``ftmi_wan_lora_ffn_block_*``, with ffn = 1 and ffn = 0), the C call against the Python composition, block parity against oracle/wan.py with
oracle.ltx.LoraLinear around the ten projections (text-to-video and, with tests/wan_i2v_reference.py, image-to-video), activation checkpointing, and two
optimiser steps.  Every parity case gives all lora_B non-zero values: with peft's zero init the A gradients are identically zero."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
TEN_REGEX = "blocks.*(to_q|to_k|to_v|to_out.0|ffn.net.0.proj|ffn.net.2)"
REAL = (1536, 12, 8960)  # Wan2.1-T2V-1.3B block geometry (D, heads, F): K = 8960 in the split down-projection, Q = 8960 in the token-reduction GEMM
G512, G576 = (256, 2, 512), (256, 2, 576)  # 576: an odd number of 64-deep K stages (9) that the four waves of a down-projection split 2, 2, 2, 3; not a multiple of 256
FFN_KEYS = ("ffn.net.0.proj.lora_A.weight", "ffn.net.0.proj.lora_B.weight", "ffn.net.2.lora_A.weight", "ffn.net.2.lora_B.weight")  # order of blk.lora_ffn


def _dev():
    return torch.device("cuda", 0)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _rope_tables(S, hd, seed=0):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(S, hd // 2, generator=g, dtype=torch.float64) * 6.283
    return (torch.cos(ang).float(), torch.sin(ang).float()), torch.polar(torch.ones_like(ang), ang).view(1, 1, S, hd // 2)


def _fix(k):
    return k.replace("ffn.proj_in.", "ffn.net.0.proj.").replace("ffn.proj_out.", "ffn.net.2.")


def _lora_keys(m):
    """{peft key (diffusers module names, no '.default'): parameter} of an oracle module wrapped below."""
    return {_fix(n.replace(".default.", ".")): p for n, p in m.named_parameters() if "lora_" in n}


def _wrap_oracle_block(blk, rank, alpha, g, b_std=0.02):
    """oracle.ltx.LoraLinear (peft's lora.Linear) around the eight attention projections and around ffn.proj_in (net.0.proj) / ffn.proj_out (net.2)."""
    from oracle import ltx

    for attn in (blk.attn1, blk.attn2):
        for t in ("to_q", "to_k", "to_v"):
            setattr(attn, t, ltx.LoraLinear(getattr(attn, t), rank, alpha))
        attn.to_out[0] = ltx.LoraLinear(attn.to_out[0], rank, alpha)
    blk.ffn.proj_in = ltx.LoraLinear(blk.ffn.proj_in, rank, alpha)
    blk.ffn.proj_out = ltx.LoraLinear(blk.ffn.proj_out, rank, alpha)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if "lora_B" in n:
                p.normal_(0, b_std, generator=g)


def _perturb(module, g):
    with torch.no_grad():
        for n, p in module.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))


def _load_block_adapters(gblk, keys, rank):
    from finetrainers_amd.wan import LORA_TARGETS

    with torch.no_grad():
        for j, n in enumerate(LORA_TARGETS):
            gblk.lora_A.data[j, :rank].copy_(keys[f"{n}.lora_A.weight"])
            gblk.lora_B.data[j, :, :rank].copy_(keys[f"{n}.lora_B.weight"])
        for p, k in zip(gblk.lora_ffn, FFN_KEYS):
            (p.data[:rank] if ".lora_A." in k else p.data[:, :rank]).copy_(keys[k])


def _block_pair(geom, rank, i2v=False, seed=0):
    """(oracle block with LoraLinear on the ten projections (base bf16 frozen, adapters fp32), MI355XWanBlock with the same weights and ten adapters)."""
    import wan_i2v_reference as ref
    from finetrainers_amd.wan import MI355XWanBlock
    from oracle import wan

    D, heads, ffn = geom
    kw = dict(num_attention_heads=heads, attention_head_dim=D // heads, ffn_dim=ffn, num_layers=1, text_dim=64)
    torch.manual_seed(seed)
    oblk = ref.WanI2VTransformerBlock(ref.WanI2VConfig(**kw)) if i2v else wan.WanTransformerBlock(wan.WanConfig(**kw))
    g = torch.Generator().manual_seed(7)
    _perturb(oblk, g)
    oblk = oblk.to(bf16)
    gblk = MI355XWanBlock(dim=D, heads=heads, ffn_dim=ffn, eps=1e-6, device=_dev(), added_kv_proj_dim=D if i2v else None)
    gblk.load_diffusers_state_dict({_fix(k): v for k, v in oblk.state_dict().items()})
    for p in oblk.parameters():
        p.requires_grad_(False)
    _wrap_oracle_block(oblk, rank, float(rank), g)
    gblk.add_adapter(rank, float(rank), ffn=True)
    _load_block_adapters(gblk, _lora_keys(oblk), rank)
    return oblk, gblk


def _inputs(B, S, T, D, seed, ti=0):
    g = torch.Generator().manual_seed(seed)
    x, enc = torch.randn(B, S, D, generator=g).to(bf16), torch.randn(B, T, D, generator=g).to(bf16)
    temb, dout = (0.5 * torch.randn(B, 6, D, generator=g)).to(bf16), torch.randn(B, S, D, generator=g).to(bf16)
    return x, enc, temb, dout, (torch.randn(B, ti, D, generator=g).to(bf16) if ti else None)


def _run_gpu(gblk, x, enc, temb, dout, rope, img=None):
    """-> (out, dx, d text, {peft key relative to the block: adapter gradient at the padded storage size})."""
    from finetrainers_amd.wan import LORA_TARGETS

    dev = _dev()
    xg, eg = x.to(dev).requires_grad_(True), enc.to(dev).requires_grad_(True)
    for p in gblk.lora_parameters():
        p.grad = None
    extra = () if img is None else (img.to(dev),)
    out = gblk(xg, eg, temb.to(dev), (rope[0].to(dev), rope[1].to(dev)), *extra)
    out.backward(dout.to(dev))
    torch.cuda.synchronize()
    grads = {}
    for j, n in enumerate(LORA_TARGETS):
        grads[f"{n}.lora_A.weight"], grads[f"{n}.lora_B.weight"] = gblk.lora_A.grad[j].clone(), gblk.lora_B.grad[j].clone()
    if gblk.lora_ffn is not None:
        for p, k in zip(gblk.lora_ffn, FFN_KEYS):
            grads[k] = p.grad.clone()
    return out.detach().clone(), xg.grad.clone(), eg.grad.clone(), grads


def _user_rank(grads, rank):
    return {k: (v[:rank] if ".lora_A." in k else v[:, :rank]).cpu() for k, v in grads.items()}


def _same(r0, r1, tag, n_grads=20):
    """out, dx, d text bit-equal; the adapter gradients within the order of their fp32 atomics (2e-6: test_lora_block_c_call_matches_the_python_composition)."""
    for i, n in enumerate(("output", "dx", "d text")):
        assert torch.equal(r0[i], r1[i]), f"{tag}: {n} differs: {_rel(r1[i], r0[i]):.2e}"
    assert set(r0[3]) == set(r1[3]) and len(r0[3]) == n_grads
    for k in r0[3]:
        d = float((r0[3][k] - r1[3][k]).norm() / r0[3][k].norm().clamp_min(1e-30))
        print(f"[wan-ffn-lora {tag}] {k} {d:.2e}")
        assert d < 2e-6, (tag, k, d)


# ---- 1: bit identity -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("geom,B,S,T", [(G512, 2, 48, 16), (G576, 1, 200, 64)])
def test_zero_ffn_up_projections_give_the_eight_adapter_bits(geom, B, S, T, native):
    """Feed-forward adapters attached with B = 0 (peft's init) contribute exactly nothing: output, dx and d text are the eight-adapter block's bits and the 16
    attention gradients agree to the order of their atomics; grad_B of both feed-forward adapters is non-zero (inside the user's rank, zero in the padding)
    and grad_A of both is exactly 0."""
    from finetrainers_amd.wan import MI355XWanBlock

    rank = 32
    _, ten = _block_pair(geom, rank)
    with torch.no_grad():
        ten.lora_ffn[1].zero_()
        ten.lora_ffn[3].zero_()
    eight = MI355XWanBlock(dim=geom[0], heads=geom[1], ffn_dim=geom[2], eps=ten.eps, device=_dev())
    eight.flat.data.copy_(ten.flat.data)
    eight.mark_updated()
    eight.add_adapter(rank, float(rank))
    eight.lora_A.data.copy_(ten.lora_A.data)
    eight.lora_B.data.copy_(ten.lora_B.data)
    ten.native = eight.native = native
    x, enc, temb, dout, _ = _inputs(B, S, T, geom[0], seed=B * 1000 + S + 1)
    rope, _ = _rope_tables(S, 128, seed=4)
    want, got = _run_gpu(eight, x, enc, temb, dout, rope), _run_gpu(ten, x, enc, temb, dout, rope)
    ffn = {k: got[3].pop(k) for k in FFN_KEYS}
    _same(want, got, f"B_ffn = 0, native={native}", n_grads=16)
    for k, g in ffn.items():
        if ".lora_A." in k:
            assert float(g.abs().max()) == 0.0, k
        else:
            assert float(g[:, :rank].abs().max()) > 0.0 and float(g[:, rank:].abs().max()) == 0.0, k


# ---- 2: the C call against the Python composition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [32, 64, 128])
@pytest.mark.parametrize("B,S,T", [(2, 48, 16), (1, 200, 64)])
@pytest.mark.parametrize("geom", [G512, G576])
def test_ffn_lora_block_c_call_matches_the_python_composition(geom, B, S, T, rank):
    """``ftmi_wan_lora_ffn_block_forward / _backward`` against the per-kernel composition issued from Python: output, dx and d text bit-identical, the 20
    adapter gradients equal up to the order of their fp32 atomics."""
    _, gblk = _block_pair(geom, rank)
    x, enc, temb, dout, _ = _inputs(B, S, T, geom[0], seed=B * 1000 + S + 7)
    rope, _ = _rope_tables(S, 128, seed=4)
    res = []
    for native in (False, True):
        gblk.native = native
        res.append(_run_gpu(gblk, x, enc, temb, dout, rope))
    _same(res[0], res[1], f"c-vs-python F={geom[2]} B={B} S={S} T={T} r={rank}")


# ---- 3, 4: parity against the bf16 CPU oracle and its fp32 evaluation ------------------------------------------------------------------------------------------
def _oracle_run(blk, cast, x, enc, temb, dout, freqs, img=None):
    for p in blk.parameters():
        p.grad = None
    xr, er = (t.to(cast).clone().requires_grad_(True) for t in (x, enc))
    out = blk(xr, er, temb.to(cast), freqs, *(() if img is None else (img.to(cast),)))
    out.backward(dout.to(cast))
    return out.detach(), xr.grad, er.grad, {k: p.grad.detach().clone() for k, p in _lora_keys(blk).items()}


def _parity(geom, B, S, T, rank, ti):
    """test_lora_block_parity's measurement and bounds (tests/test_gpu_wan_lora.py), over 20 gradient tensors."""
    from oracle import ltx

    oblk, gblk = _block_pair(geom, rank, i2v=ti > 0)
    x, enc, temb, dout, img = _inputs(B, S, T, geom[0], seed=B * 1000 + S, ti=ti)
    rope, freqs = _rope_tables(S, 128, seed=3)
    o_ref, dx_ref, de_ref, g_ref = _oracle_run(oblk, bf16, x, enc, temb, dout, freqs, img)
    o32, dx32, de32, g32 = _oracle_run(copy.deepcopy(oblk).float(), torch.float32, x, enc, temb, dout, freqs, img)
    floor, floor_worst = ltx.grads_rel_l2(g_ref, g32)
    out, dx, de, grads = _run_gpu(gblk, x, enc, temb, dout, rope, img)
    got = _user_rank(grads, rank)
    assert set(got) == set(g_ref) and len(got) == 20
    glob, worst = ltx.grads_rel_l2(got, g_ref)
    glob32, worst32 = ltx.grads_rel_l2(got, g32)
    e_o, e_dx, e_de = _rel(out, o_ref), _rel(dx, dx_ref), _rel(de, de_ref)
    print(f"[wan-ffn-lora block D={geom[0]} F={geom[2]} B={B} S={S} T={T} TI={ti} r={rank}] out {e_o:.2e} (oracle bf16 vs fp32 {_rel(o_ref, o32):.2e}) | dx {e_dx:.2e} "
          f"({_rel(dx_ref, dx32):.2e}) d text {e_de:.2e} ({_rel(de_ref, de32):.2e}) | adapter grads vs bf16 oracle {glob:.2e} (worst {worst:.2e}), vs fp32 oracle "
          f"{glob32:.2e} (worst {worst32:.2e}); bf16 oracle vs fp32 oracle {floor:.2e} (worst {floor_worst:.2e})")
    for k in FFN_KEYS:
        print(f"    {k}: vs bf16 oracle {_rel(got[k], g_ref[k]):.2e}, vs fp32 oracle {_rel(got[k], g32[k]):.2e}, bf16 oracle vs fp32 oracle {_rel(g_ref[k], g32[k]):.2e}")
    assert e_o < 5e-3 and e_dx < 1e-2
    assert glob < 2.0 * floor + 2e-3 and worst < 2.0 * floor_worst + 5e-3
    assert glob32 < 1.5 * floor + 1e-3 and worst32 < 1.5 * floor_worst + 2e-3


@pytest.mark.parametrize("geom,B,S,T,rank", [(G512, 2, 48, 16, 32), (G576, 1, 200, 64, 128), (REAL, 1, 200, 64, 32)])
def test_ffn_lora_block_parity(geom, B, S, T, rank):
    """One block, forward + backward, against the bf16 CPU oracle with peft-style LoraLinear on the ten projections and against its fp32 evaluation (the
    floor = the bf16 oracle's own distance from fp32, measured here).  The last case runs the real widths: the down-projections of ffn.net.2's adapter and of
    d pre contract over 8960 columns, dA of ffn.net.2 is a [64, 8960] token reduction."""
    _parity(geom, B, S, T, rank, ti=0)


def test_ffn_lora_block_parity_with_the_image_context():
    """Image-to-video: TI = 257 image tokens in attn2 next to the ten adapters, against tests/wan_i2v_reference.py's block wrapped the same way."""
    _parity(G512, 2, 48, 16, 32, ti=257)


# ---- 5: activation checkpointing ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("geom,ti", [(G576, 0), (G512, 257)])
def test_ffn_lora_block_recomputation(geom, ti, native):
    """Gradient checkpointing (the block keeps its input only; the forward with out = NULL refills what the backward reads, net.2's down-projected rows
    included): the same output, dx and d text bits, the same 20 gradients to the order of their atomics."""
    _, gblk = _block_pair(geom, 32, i2v=ti > 0)
    gblk.native = native
    x, enc, temb, dout, img = _inputs(1, 200, 64, geom[0], seed=31, ti=ti)
    rope, _ = _rope_tables(200, 128, seed=4)
    kept = _run_gpu(gblk, x, enc, temb, dout, rope, img)
    gblk.gradient_checkpointing = True
    _same(kept, _run_gpu(gblk, x, enc, temb, dout, rope, img), f"recomputed, native={native}, TI={ti}")


# ---- 6: model and step -------------------------------------------------------------------------------------------------------------------------------------
SMALL = dict(num_attention_heads=2, attention_head_dim=128, ffn_dim=512, text_dim=64)


def _model_pair(layers, rank=32, alpha=32.0, seed=0):
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig
    from oracle import wan

    torch.manual_seed(seed)
    omodel = wan.WanTransformer3DModel(wan.WanConfig(num_layers=layers, **SMALL))
    g = torch.Generator().manual_seed(7)
    _perturb(omodel, g)
    omodel = omodel.to(bf16)
    gmodel = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, **SMALL), device=_dev())
    gmodel.load_diffusers_state_dict({_fix(k): v for k, v in omodel.state_dict().items()})
    for p in omodel.parameters():
        p.requires_grad_(False)
    for blk in omodel.blocks:
        _wrap_oracle_block(blk, rank, alpha, g)
    gmodel.add_adapter(rank, alpha, target_modules=TEN_REGEX)
    gmodel.load_lora_state_dict({k: v.detach() for k, v in _lora_keys(omodel).items()})
    return omodel, gmodel


def _batch(B=2, seed=11, text_dim=64):
    g = torch.Generator().manual_seed(seed)
    C, F_, H, W = 16, 2, 8, 12  # 2 x 4 x 6 = 48 tokens
    moments = torch.randn(B, 2 * C, F_, H, W, generator=g).to(bf16)
    moments[:, C:] = (moments[:, C:].float() * 0.3 - 2.0).to(bf16)
    return dict(moments=moments, text=torch.randn(B, 16, text_dim, generator=g).to(bf16), eps=torch.randn(B, C, F_, H, W, generator=g).to(bf16),
                noise=torch.randn(B, C, F_, H, W, generator=g).to(bf16), sigmas=torch.tensor([0.23, 0.81][:B]),
                mean=0.1 * torch.randn(C, generator=g), std=1.0 + 0.2 * torch.rand(C, generator=g))


def test_ffn_lora_step_two_steps_against_the_oracle(tmp_path):
    """Two ``MI355XWanLoRAStep`` steps at 2 layers against torch AdamW over the wrapped oracle's 40 adapter parameters with the reference's clip: loss and
    pre-clip gradient norm within test_lora_step_two_steps_against_the_oracle's bounds at both steps; every adapter tensor moved, every padded entry of the
    storage is still exactly 0; the saved adapters loaded into a fresh model give the same prediction bits."""
    from finetrainers_amd import wire
    from finetrainers_amd.wan import MI355XWanLoRAStep, MI355XWanSpecOps
    from oracle import ltx, wan

    dev = _dev()
    rank = 32
    omodel, gmodel = _model_pair(2, rank=rank)
    b = _batch()
    base_before = [gmodel.root.data.clone()] + [blk.flat.data.clone() for blk in gmodel.blocks]
    lora_before = {k: v.clone() for k, v in gmodel.lora_state_dict().items()}
    assert len(lora_before) == 40
    kw = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-2)
    oparams = [p for p in omodel.parameters() if p.requires_grad]
    assert len(oparams) == 40
    opt = torch.optim.AdamW(oparams, fused=False, **kw)
    step = MI355XWanLoRAStep(gmodel, max_grad_norm=1.0, **kw)
    assert step.flat.numel() == sum(p.numel() for p in gmodel.lora_parameters()) and len(gmodel.lora_parameters()) == 12
    args = (b["moments"].to(dev), b["text"].to(dev), b["mean"].to(dev), b["std"].to(dev), b["sigmas"].to(dev))
    for it in range(2):
        pred, target, _ = wan.spec_forward(omodel, b["moments"], b["mean"], b["std"], b["text"], b["sigmas"].view(-1, 1, 1, 1, 1), b["eps"], b["noise"])
        loss_ref = wan.sft_loss(pred, target, b["sigmas"])
        loss_ref.backward()
        gn_ref = float(ltx.clip_grad_norm_(oparams, 1.0))
        opt.step()
        opt.zero_grad()
        out = step.step(*args, posterior_noise=b["eps"].to(dev), noise=b["noise"].to(dev))
        torch.cuda.synchronize()
        print(f"[wan-ffn-lora step {it}] loss {out['loss'].item():.6f} vs {loss_ref.item():.6f}; grad_norm {out['grad_norm'].item():.5e} vs oracle {gn_ref:.5e}")
        assert abs(out["loss"].item() - loss_ref.item()) < 2e-3 * abs(loss_ref.item()) and abs(out["grad_norm"].item() - gn_ref) < 1e-2 * gn_ref
    base_after = [gmodel.root.data] + [blk.flat.data for blk in gmodel.blocks]
    assert all(torch.equal(a, c) for a, c in zip(base_before, base_after)), "the frozen base moved"
    after = gmodel.lora_state_dict()
    assert all(not torch.equal(after[k], lora_before[k]) for k in after), "an adapter tensor did not move"
    for blk in gmodel.blocks:  # the padding of every stored tensor (ranks 32 .. 63)
        assert float(blk.lora_A.data[:, rank:].abs().max()) == 0.0 and float(blk.lora_B.data[:, :, rank:].abs().max()) == 0.0
        for p, k in zip(blk.lora_ffn, FFN_KEYS):
            assert float((p.data[rank:] if ".lora_A." in k else p.data[:, rank:]).abs().max()) == 0.0, k
    num = den = 0.0
    okeys = _lora_keys(omodel)
    for k, v in after.items():  # the UPDATES against torch.optim.AdamW on the oracle's adapters
        upd, upd_ref = v.cpu() - lora_before[k].cpu(), okeys[k].detach() - lora_before[k].cpu()
        num += float((upd - upd_ref).pow(2).sum())
        den += float(upd_ref.pow(2).sum())
    print(f"[wan-ffn-lora step] adapter update vs torch.optim.AdamW on the oracle: rel L2 {math.sqrt(num / den):.3e}")
    assert step.state_dict()["step"] == 2
    wire.save_lora_weights(str(tmp_path), gmodel.lora_state_dict(), wire.lora_config_metadata(rank, 32.0, TEN_REGEX))
    loaded, cfg = wire.load_lora_weights(str(tmp_path))
    _, fresh = _model_pair(2, rank=cfg["r"], alpha=cfg["lora_alpha"])
    fresh.load_lora_state_dict(loaded)
    ops_spec = MI355XWanSpecOps()
    preds = []
    for m in (gmodel, fresh):
        with torch.no_grad():
            pred, _, _ = ops_spec.forward(m, b["moments"].to(dev), b["text"].to(dev), b["sigmas"].to(dev), b["mean"].to(dev), b["std"].to(dev),
                                          posterior_noise=b["eps"].to(dev), noise=b["noise"].to(dev))
        preds.append(pred.clone())
    assert cfg["target_modules"] == TEN_REGEX and torch.equal(preds[0], preds[1])
