"""Wan-T2V LoRA fine-tuning over a frozen base (the reference's Wan SFT recipes: --training_type lora --rank 32 --lora_alpha 32
--target_modules "blocks.*(to_q|to_k|to_v|to_out.0)") on the GPU: the frozen path against the full fine-tune's bits, the C call against the Python
composition, block / model / step parity against oracle/wan.py with oracle.ltx.LoraLinear around the attention projections.  Every parity case gives
lora_B non-zero values: with peft's zero init the A gradients are identically zero."""
import copy
import math
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
RECIPE_REGEX = "blocks.*(to_q|to_k|to_v|to_out.0)"
REAL = (1536, 12, 8960)  # Wan2.1-T2V-1.3B block geometry (D, H, F)


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


def _wrap_oracle_attention(attn, rank, alpha, g, b_std=0.02):
    from oracle import ltx

    for t in ("to_q", "to_k", "to_v"):
        setattr(attn, t, ltx.LoraLinear(getattr(attn, t), rank, alpha))
    attn.to_out[0] = ltx.LoraLinear(attn.to_out[0], rank, alpha)
    with torch.no_grad():
        for n, p in attn.named_parameters():
            if "lora_B" in n:
                p.normal_(0, b_std, generator=g)


def _lora_keys(model_or_block):
    """{peft key without '.default': parameter} of an oracle module wrapped above."""
    return {n.replace(".default.", "."): p for n, p in model_or_block.named_parameters() if "lora_" in n}


def _block_pair(geom=(256, 2, 512), rank=32, alpha=32.0, seed=0):
    """(oracle block with LoraLinear on the eight projections (base bf16 frozen, adapters fp32), MI355XWanBlock with the same weights and adapters)."""
    from finetrainers_amd.wan import LORA_TARGETS, MI355XWanBlock
    from oracle import wan

    D, heads, ffn = geom
    cfg = wan.WanConfig(num_attention_heads=heads, attention_head_dim=D // heads, ffn_dim=ffn, num_layers=1, text_dim=64)
    torch.manual_seed(seed)
    oblk = wan.WanTransformerBlock(cfg)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in oblk.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    oblk = oblk.to(bf16)
    gblk = MI355XWanBlock(dim=D, heads=heads, ffn_dim=ffn, eps=cfg.eps, device=_dev())
    gblk.load_diffusers_state_dict({_fix(k): v for k, v in oblk.state_dict().items()})
    for p in oblk.parameters():
        p.requires_grad_(False)
    if rank:
        for attn in (oblk.attn1, oblk.attn2):
            _wrap_oracle_attention(attn, rank, alpha, g)
        gblk.add_adapter(rank, alpha)
        keys = _lora_keys(oblk)
        with torch.no_grad():
            for j, n in enumerate(LORA_TARGETS):
                gblk.lora_A.data[j, :rank].copy_(keys[f"{n}.lora_A.weight"])
                gblk.lora_B.data[j, :, :rank].copy_(keys[f"{n}.lora_B.weight"])
    else:
        gblk.freeze_base()
    return oblk, gblk


def _block_inputs(B, S, T, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, D, generator=g).to(bf16)
    enc = torch.randn(B, T, D, generator=g).to(bf16)
    temb = (0.5 * torch.randn(B, 6, D, generator=g)).to(bf16)
    dout = torch.randn(B, S, D, generator=g).to(bf16)
    return x, enc, temb, dout


def _run_gpu_block(gblk, x, enc, temb, dout, rope, enc_grad=True):
    dev = _dev()
    xg = x.to(dev).requires_grad_(True)
    eg = enc.to(dev).requires_grad_(enc_grad)
    tg = temb.to(dev)
    if gblk.lora_A is not None:
        gblk.lora_A.grad = gblk.lora_B.grad = None
    out = gblk(xg, eg, tg, (rope[0].to(dev), rope[1].to(dev)))
    out.backward(dout.to(dev))
    torch.cuda.synchronize()
    ga = None if gblk.lora_A is None else gblk.lora_A.grad.clone()
    gb = None if gblk.lora_B is None else gblk.lora_B.grad.clone()
    return out.detach().clone(), xg.grad.clone(), (eg.grad.clone() if enc_grad else None), ga, gb


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("geom,B,S,T", [((256, 2, 512), 2, 48, 16), (REAL, 1, 200, 64)])
def test_frozen_path_has_the_full_finetune_bits(geom, B, S, T, native):
    """r = 0 and (r = 32, B = 0): the LoRA block's output is the full fine-tune block's, bit for bit; with r = 0 its dx (and d text) is the full
    fine-tune backward's.  Through the C calls (``native``) and through the Python walk, both blocks the same way."""
    from finetrainers_amd.wan import MI355XWanBlock

    _, frozen = _block_pair(geom, rank=0)
    full = MI355XWanBlock(dim=geom[0], heads=geom[1], ffn_dim=geom[2], eps=frozen.eps, device=_dev())
    frozen.native = full.native = native
    full.flat.data.copy_(frozen.flat.data)
    full.mark_updated()
    x, enc, temb, dout = _block_inputs(B, S, T, geom[0], seed=B * 1000 + S + 1)
    rope, _ = _rope_tables(S, 128, seed=4)
    dev = _dev()
    full.zero_grad_flat()
    xg, eg = x.to(dev).requires_grad_(True), enc.to(dev).requires_grad_(True)
    out_full = full(xg, eg, temb.to(dev).requires_grad_(True), (rope[0].to(dev), rope[1].to(dev)))
    out_full.backward(dout.to(dev))
    torch.cuda.synchronize()
    out0, dx0, de0, _, _ = _run_gpu_block(frozen, x, enc, temb, dout, rope)
    assert torch.equal(out0, out_full.detach()), f"r = 0 output: {_rel(out0, out_full.detach()):.2e}"
    assert torch.equal(dx0, xg.grad), f"r = 0 dx: {_rel(dx0, xg.grad):.2e}"
    assert torch.equal(de0, eg.grad), f"r = 0 d text: {_rel(de0, eg.grad):.2e}"
    frozen.add_adapter(32, 32.0)  # peft's init: B = 0 -- the adapters contribute exactly nothing
    out32, _, _, ga, gb = _run_gpu_block(frozen, x, enc, temb, dout, rope)
    assert torch.equal(out32, out_full.detach()), f"r = 32, B = 0 output: {_rel(out32, out_full.detach()):.2e}"
    assert float(ga.abs().max()) == 0.0 and float(gb[:, :, :32].abs().max()) > 0.0 and float(gb[:, :, 32:].abs().max()) == 0.0


@pytest.mark.parametrize("B,S,T", [(2, 48, 16), (1, 200, 64), (2, 320, 40)])
@pytest.mark.parametrize("rank", [32, 64])
def test_lora_block_c_call_matches_the_python_composition(B, S, T, rank):
    """``ftmi_wan_lora_ffn_block_forward / _backward`` (TI = 0, ffn = 0) against the per-kernel composition issued from Python: output, dx and d text bit-identical, the 16
    adapter gradients equal up to the order of their fp32 atomics (the bound of test_wan_block_c_call_matches_the_python_composition)."""
    _, gblk = _block_pair((256, 2, 512), rank=rank, alpha=float(rank))
    x, enc, temb, dout = _block_inputs(B, S, T, 256, seed=B * 1000 + S + 7)
    rope, _ = _rope_tables(S, 128, seed=4)
    res = []
    for native in (False, True):
        gblk.native = native
        res.append(_run_gpu_block(gblk, x, enc, temb, dout, rope))
    r0, r1 = res
    for i, n in enumerate(("output", "dx", "d text")):
        assert torch.equal(r0[i], r1[i]), f"{n} differs: {_rel(r1[i], r0[i]):.2e}"
    for i, n in ((3, "lora_A"), (4, "lora_B")):
        for j in range(8):
            d = float((r0[i][j] - r1[i][j]).norm() / r0[i][j].norm().clamp_min(1e-30))
            print(f"[wan-lora c-vs-python B={B} S={S} T={T} r={rank}] {n}[{j}] {d:.2e}")
            assert d < 2e-6, (n, j, d)


def _oracle_block_run(blk, cast, x, enc, temb, dout, freqs):
    for p in blk.parameters():
        p.grad = None
    xr, er = (t.to(cast).clone().requires_grad_(True) for t in (x, enc))
    out = blk(xr, er, temb.to(cast), freqs)
    out.backward(dout.to(cast))
    return out.detach(), xr.grad, er.grad, {k: p.grad.detach().clone() for k, p in _lora_keys(blk).items()}


def _gpu_lora_grads(ga, gb, rank):
    from finetrainers_amd.wan import LORA_TARGETS

    out = {}
    for j, n in enumerate(LORA_TARGETS):
        out[f"{n}.lora_A.weight"] = ga[j, :rank].cpu()
        out[f"{n}.lora_B.weight"] = gb[j, :, :rank].cpu()
    return out


@pytest.mark.parametrize("rank", [32, 64])
@pytest.mark.parametrize("B,S,T,geom", [(2, 48, 16, (256, 2, 512)), (1, 200, 64, (256, 2, 512)), (1, 20280, 512, REAL)])
def test_lora_block_parity(B, S, T, geom, rank):
    """One block, forward + backward, against the bf16 CPU oracle with peft-style LoraLinear on the eight projections and against its fp32 evaluation
    (the floor = the bf16 oracle's own distance from fp32, measured here).  The last case is the recipe's bucket at its real size: 49 x 480 x 832 ->
    20 280 = 13 x 30 x 52 video tokens (ragged for the 64-wide key tiles) + 512 text tokens at the 1.3 B geometry.  Only that case may skip, under the
    oracle time budget FTMI_ORACLE_BUDGET_S (test_full_depth_config2_parity's guard), and says so."""
    from oracle import ltx

    oblk, gblk = _block_pair(geom, rank=rank, alpha=float(rank))
    D = geom[0]
    x, enc, temb, dout = _block_inputs(B, S, T, D, seed=B * 1000 + S)
    rope, freqs = _rope_tables(S, 128, seed=3)
    if S > 4096:
        budget = float(os.environ.get("FTMI_ORACLE_BUDGET_S", "480"))
        s1 = S // 10
        _, f1 = _rope_tables(s1, 128, seed=3)
        t0 = time.time()
        _oracle_block_run(oblk, bf16, x[:, :s1], enc, temb, dout[:, :s1], f1)
        est = (time.time() - t0) * 10 * 1.5 * 2.5  # ten times the tokens (attention grows faster: x 1.5), bf16 + fp32 (the slower of the two)
        print(f"[wan-lora block] oracle estimate for S={S}: {est:.0f} s on {torch.get_num_threads()} threads (budget {budget:.0f} s)")
        if est > budget:
            pytest.skip(f"real-size LoRA block parity NOT run: the host oracle would need ~{est:.0f} s, beyond FTMI_ORACLE_BUDGET_S={budget:.0f} s")
    o_ref, dx_ref, de_ref, g_ref = _oracle_block_run(oblk, bf16, x, enc, temb, dout, freqs)
    o32, dx32, de32, g32 = _oracle_block_run(copy.deepcopy(oblk).float(), torch.float32, x, enc, temb, dout, freqs)
    floor, floor_worst = ltx.grads_rel_l2(g_ref, g32)
    out, dx, de, ga, gb = _run_gpu_block(gblk, x, enc, temb, dout, rope)
    got = _gpu_lora_grads(ga, gb, rank)
    assert set(got) == set(g_ref) and len(got) == 16
    glob, worst = ltx.grads_rel_l2(got, g_ref)
    glob32, worst32 = ltx.grads_rel_l2(got, g32)
    e_o, e_dx, e_de = _rel(out, o_ref), _rel(dx, dx_ref), _rel(de, de_ref)
    print(f"[wan-lora block B={B} S={S} T={T} r={rank}] out {e_o:.2e} (oracle bf16 vs fp32 {_rel(o_ref, o32):.2e}) | dx {e_dx:.2e} ({_rel(dx_ref, dx32):.2e}) "
          f"d text {e_de:.2e} ({_rel(de_ref, de32):.2e}) | adapter grads vs bf16 oracle {glob:.2e} (worst {worst:.2e}), vs fp32 oracle {glob32:.2e} "
          f"(worst {worst32:.2e}); bf16 oracle vs fp32 oracle {floor:.2e} (worst {floor_worst:.2e})")
    assert e_o < 5e-3 and e_dx < 1e-2
    assert glob < 2.0 * floor + 2e-3 and worst < 2.0 * floor_worst + 5e-3
    assert glob32 < 1.5 * floor + 1e-3 and worst32 < 1.5 * floor_worst + 2e-3


@pytest.mark.parametrize("native", [True, False])
def test_frozen_text_embedder_skips_denc_with_the_same_bits(native):
    """denc = NULL (no gradient wanted on the text rows): same dx and adapter-gradient bits as with denc."""
    _, gblk = _block_pair((256, 2, 512), rank=32)
    gblk.native = native
    x, enc, temb, dout = _block_inputs(2, 200, 40, 256, seed=21)
    rope, _ = _rope_tables(200, 128, seed=4)
    with_denc = _run_gpu_block(gblk, x, enc, temb, dout, rope, enc_grad=True)
    without = _run_gpu_block(gblk, x, enc, temb, dout, rope, enc_grad=False)
    assert without[2] is None and torch.equal(with_denc[0], without[0]) and torch.equal(with_denc[1], without[1])
    # the adapter gradients are sums of fp32 atomics: their order is not fixed from run to run, the operands are identical
    for i in (3, 4):
        assert _rel(without[i], with_denc[i]) < 2e-6


def _model_pair(layers, kw, rank=32, alpha=32.0, seed=0, perturb=True):
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig
    from oracle import wan

    torch.manual_seed(seed)
    omodel = wan.WanTransformer3DModel(wan.WanConfig(num_layers=layers, **kw))
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in omodel.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif perturb and n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    omodel = omodel.to(bf16)
    gmodel = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, **kw), device=_dev())
    gmodel.load_diffusers_state_dict({_fix(k): v for k, v in omodel.state_dict().items()})
    for p in omodel.parameters():
        p.requires_grad_(False)
    for blk in omodel.blocks:
        for attn in (blk.attn1, blk.attn2):
            _wrap_oracle_attention(attn, rank, alpha, g)
    gmodel.add_adapter(rank, alpha, target_modules=RECIPE_REGEX)
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


def _oracle_model_run(model, cast, b):
    from oracle import wan

    for p in model.parameters():
        p.grad = None
    pred, target, _ = wan.spec_forward(model, b["moments"].to(cast), b["mean"], b["std"], b["text"].to(cast), b["sigmas"].view(-1, 1, 1, 1, 1), b["eps"].to(cast),
                                       b["noise"].to(cast))
    loss = wan.sft_loss(pred, target, b["sigmas"])
    loss.backward()
    return loss.item(), pred.detach(), {k: p.grad.detach().clone() for k, p in _lora_keys(model).items()}


def _gpu_model_run(gmodel, b):
    from finetrainers_amd.wan import MI355XWanSpecOps

    dev = _dev()
    spec = MI355XWanSpecOps()
    for p in gmodel.lora_parameters():
        p.grad = None
    pred, target, _ = spec.forward(gmodel, b["moments"].to(dev), b["text"].to(dev), b["sigmas"].to(dev), b["mean"].to(dev), b["std"].to(dev),
                                   posterior_noise=b["eps"].to(dev), noise=b["noise"].to(dev))
    loss = spec.loss_backward(pred, target)
    torch.cuda.synchronize()
    return loss.item(), pred.detach().clone(), {k: v.detach().cpu().clone() for k, v in gmodel.lora_grad_state_dict().items()}


def test_lora_model_full_depth_parity_1_3b_architecture():
    """The 1.3 B architecture at its full 30 blocks (width 1536, feed-forward 8960, 4096-wide text embeddings) on a small clip, rank 32 on all 240
    projections: loss and prediction within test_wan_model_full_depth_parity_config4_architecture's bounds, the 480 adapter-gradient tensors within the
    floor form (floor = the bf16 oracle against its fp32 evaluation, measured here)."""
    from oracle import ltx

    omodel, gmodel = _model_pair(30, {}, rank=32, alpha=32.0, perturb=False)
    b = _batch(B=1, text_dim=4096)
    b["sigmas"] = b["sigmas"][:1]
    loss_ref, pred_ref, g_ref = _oracle_model_run(omodel, bf16, b)
    o32 = copy.deepcopy(omodel).float()
    loss32, pred32, g32 = _oracle_model_run(o32, torch.float32, b)
    del o32
    floor, floor_worst = ltx.grads_rel_l2(g_ref, g32)
    loss, pred, got = _gpu_model_run(gmodel, b)
    assert set(got) == set(g_ref) and len(got) == 480
    glob, worst = ltx.grads_rel_l2(got, g_ref)
    glob32, worst32 = ltx.grads_rel_l2(got, g32)
    e_pred, e_loss = _rel(pred, pred_ref), abs(loss - loss_ref) / abs(loss_ref)
    print(f"[wan-lora model 1.3B, 30 blocks] pred {e_pred:.2e} (oracle bf16 vs fp32 {_rel(pred_ref, pred32):.2e}) loss {loss:.6f} vs {loss_ref:.6f} (fp32 {loss32:.6f}, "
          f"rel {e_loss:.2e}) | 480 adapter gradients vs bf16 oracle {glob:.2e} (worst {worst:.2e}), vs fp32 oracle {glob32:.2e} (worst {worst32:.2e}); "
          f"bf16 oracle vs fp32 oracle {floor:.2e} (worst {floor_worst:.2e})")
    assert e_pred < 2e-2 and e_loss < 3e-3
    assert glob < 2.0 * floor + 2e-3 and worst < 2.0 * floor_worst + 5e-3
    assert glob32 < 1.5 * floor + 1e-3 and worst32 < 1.5 * floor_worst + 2e-3


SMALL = dict(num_attention_heads=2, attention_head_dim=128, ffn_dim=512, text_dim=64)


@pytest.mark.parametrize("native", [True, False])
def test_activation_checkpointing_same_loss_and_prediction_bits(native):
    """``apply_activation_checkpointing()``: every block keeps only its input and refills its saved activations in the backward.  Loss and prediction
    bit-identical; the adapter gradients agree to the order of their fp32 atomics (issued in a different grouping), not bit for bit."""
    _, gmodel = _model_pair(3, SMALL)
    for blk in gmodel.blocks:
        blk.native = native
    b = _batch()
    loss0, pred0, g0 = _gpu_model_run(gmodel, b)
    gmodel.apply_activation_checkpointing()
    assert all(blk.gradient_checkpointing for blk in gmodel.blocks)
    loss1, pred1, g1 = _gpu_model_run(gmodel, b)
    assert loss0 == loss1 and torch.equal(pred0, pred1)
    for k in g0:
        d = float((g0[k] - g1[k]).norm() / g0[k].norm().clamp_min(1e-30))
        assert d < 2e-6, (k, d)


def test_lora_step_two_steps_against_the_oracle(tmp_path):
    """Two ``MI355XWanLoRAStep`` steps against torch AdamW over the wrapped oracle's adapter parameters with the reference's clip (oracle.ltx.clip_grad_norm_):
    loss and pre-clip gradient norm within test_wan_full_finetune_step_single_gpu's bounds at both steps; afterwards the base buffers are bit-unchanged and
    only adapters moved; the saved adapters loaded into a fresh model give the same prediction bits."""
    from finetrainers_amd import wire
    from finetrainers_amd.wan import MI355XWanLoRAStep, MI355XWanModelSpecification, MI355XWanSpecOps
    from oracle import ltx, wan

    dev = _dev()
    omodel, gmodel = _model_pair(2, SMALL)
    b = _batch()
    base_before = [gmodel.root.data.clone()] + [blk.flat.data.clone() for blk in gmodel.blocks]
    lora_before = {k: v.clone() for k, v in gmodel.lora_state_dict().items()}
    kw = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-2)
    oparams = [p for p in omodel.parameters() if p.requires_grad]
    assert len(oparams) == 32
    opt = torch.optim.AdamW(oparams, fused=False, **kw)
    step = MI355XWanLoRAStep(gmodel, max_grad_norm=1.0, **kw)
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
        print(f"[wan-lora step {it}] loss {out['loss'].item():.6f} vs {loss_ref.item():.6f}; grad_norm {out['grad_norm'].item():.5e} vs oracle {gn_ref:.5e}")
        assert abs(out["loss"].item() - loss_ref.item()) < 2e-3 * abs(loss_ref.item()) and abs(out["grad_norm"].item() - gn_ref) < 1e-2 * gn_ref
    base_after = [gmodel.root.data] + [blk.flat.data for blk in gmodel.blocks]
    assert all(torch.equal(a, c) for a, c in zip(base_before, base_after)), "the frozen base moved"
    after = gmodel.lora_state_dict()
    assert all(not torch.equal(after[k], lora_before[k]) for k in after), "an adapter tensor did not move"
    assert all(float(blk.lora_A.data[:, 32:].abs().max()) == 0.0 and float(blk.lora_B.data[:, :, 32:].abs().max()) == 0.0 for blk in gmodel.blocks)
    num = den = 0.0
    okeys = _lora_keys(omodel)
    for k, v in after.items():  # the UPDATES against torch.optim.AdamW on the oracle's adapters
        upd, upd_ref = v.cpu() - lora_before[k].cpu(), okeys[k].detach() - lora_before[k].cpu()
        num += float((upd - upd_ref).pow(2).sum())
        den += float(upd_ref.pow(2).sum())
    print(f"[wan-lora step] adapter update vs torch.optim.AdamW on the oracle: rel L2 {math.sqrt(num / den):.3e}")
    sd = step.state_dict()
    assert sd["step"] == 2 and step.step_count == 2
    # save -> load into a fresh model -> same prediction bits
    spec = MI355XWanModelSpecification(pretrained_model_name_or_path=None)
    spec._save_lora_weights(str(tmp_path), gmodel.lora_state_dict(), scheduler=None, metadata=wire.lora_config_metadata(32, 32.0, RECIPE_REGEX))
    loaded, cfg = wire.load_lora_weights(str(tmp_path))
    _, fresh = _model_pair(2, SMALL)
    fresh.load_lora_state_dict(loaded)
    ops_spec = MI355XWanSpecOps()
    preds = []
    for m in (gmodel, fresh):
        with torch.no_grad():
            pred, _, _ = ops_spec.forward(m, b["moments"].to(dev), b["text"].to(dev), b["sigmas"].to(dev), b["mean"].to(dev), b["std"].to(dev),
                                          posterior_noise=b["eps"].to(dev), noise=b["noise"].to(dev))
        preds.append(pred.clone())
    assert cfg["r"] == 32 and torch.equal(preds[0], preds[1])
