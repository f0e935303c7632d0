"""CogVideoX gradient checkpointing on the GPU (ftmi_cog_config.checkpoint = 1: one block slot, the backward runs a block's forward launches again up to the
feed-forward's pre-activation): the same prediction bit for bit and the same LoRA gradients as the kept-activation step, in block ranges with the bucket
hook, at one block, through the C ABI with a sentinel in the caller's output, against oracle/cogvideox.py, and from less memory.  pytest -m gpu."""

import copy
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
KW = dict(sample_width=12, sample_height=8, sample_frames=9, max_text_seq_length=16)  # latents [2, 3, 16, 8, 12] -> 72 video + 16 text = 88 joint tokens (ragged vs 64)


def _dev():
    return torch.device("cuda", 0)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@functools.lru_cache(maxsize=None)
def _model(layers, rotary):
    """(model, oracle model) at width 1920, rank 64; built once per geometry, the tests only flip the model's flags and put them back."""
    from finetrainers_amd.cogvideox import CogVideoXTransformerConfig, MI355XCogVideoXTransformer3DModel
    from oracle import cogvideox as cvx

    kw = dict(KW, num_layers=layers, use_rotary_positional_embeddings=bool(rotary))
    if rotary == "1.5":
        kw.update(patch_size_t=2, ofs_embed_dim=512, patch_bias=False)
    omodel = cvx.build_model(cvx.CogVideoXConfig(**kw), seed=0, rank=64, alpha=64.0, lora_b_std=0.02)
    with torch.no_grad():
        g = torch.Generator().manual_seed(7)
        for n, p in omodel.named_parameters():
            if "norm" in n and "linear" not in n and p.dim() == 1:
                p.copy_(((1.0 if n.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g)).to(p.dtype))
    sd = {k.replace("ff.proj_in.", "ff.net.0.proj.").replace("ff.proj_out.", "ff.net.2."): v for k, v in omodel.state_dict().items()}
    m = MI355XCogVideoXTransformer3DModel(CogVideoXTransformerConfig(**kw), device=_dev())
    m.load_diffusers_state_dict(sd)
    m.add_adapter(r=64, lora_alpha=64.0)
    m.load_lora_state_dict({k: v for k, v in sd.items() if "lora_" in k})
    return m, omodel


@functools.lru_cache(maxsize=None)
def _batch():
    g = torch.Generator().manual_seed(4)
    dev = _dev()
    lat = torch.randn(2, 3, 16, 8, 12, generator=g).to(bf16).to(dev)
    noise = torch.randn(2, 3, 16, 8, 12, generator=g).to(bf16).to(dev)
    text = torch.randn(2, 16, 4096, generator=g).to(bf16).to(dev)
    return lat, noise, text, torch.tensor([0.35, 0.8], device=dev)


def _run(m, ckpt, clear=True):
    """One forward + backward through the specification ops -> (pred, loss, flat LoRA gradient)."""
    from finetrainers_amd.cogvideox import MI355XCogVideoXSpecOps

    lat, noise, text, sig = _batch()
    spec = MI355XCogVideoXSpecOps()
    m.enable_gradient_checkpointing() if ckpt else m.disable_gradient_checkpointing()
    try:
        if clear:
            for blk in m.transformer_blocks:
                blk.lora_A.grad = blk.lora_B.grad = None
        pred, target, _ = spec.forward(m, lat, text, sig, noise=noise)
        loss = spec.loss_backward(pred, target, sig)
        torch.cuda.synchronize()
        return pred.detach().clone(), loss.item(), m.flat_lora_grad().clone()
    finally:
        m.disable_gradient_checkpointing()


def _same_step(layers, rotary):
    m, _ = _model(layers, rotary)
    pred0, loss0, g0 = _run(m, False)
    pred1, loss1, g1 = _run(m, True)
    e = _rel(g1, g0)
    print(f"[cog-ckpt L={layers} rotary={rotary}] flat LoRA gradient, checkpointed vs kept: rel L2 {e:.3e}; loss {loss1:.6f} vs {loss0:.6f}")
    assert torch.equal(pred1, pred0), "the forward issues the same launches"
    assert g0.norm().item() > 0 and torch.isfinite(g1).all()
    assert e < 1e-6  # the input-gradient chain is the same launches on the same bits; only the weight-gradient launches are batched differently (fp32 atomics)


@pytest.mark.parametrize("rotary", [True, False])
def test_checkpointed_step_equals_the_kept_activation_step(rotary):
    _same_step(3, rotary)


def test_one_block_has_no_hidden_state_slot():
    """L = 1: block L - 1 is block 0 -- it reads the caller's tokens and its output is the caller's buffer."""
    _same_step(1, True)


def test_block_ranges_with_the_bucket_hook():
    m, _ = _model(3, True)
    _, _, g_one = _run(m, True)
    seen = []
    m._grad_bucket_hook, m.grad_bucket_blocks = (lambda lo, hi, ga, gb: seen.append((lo, hi, tuple(ga.shape), tuple(gb.shape)))), 2
    try:
        _, _, g_rng = _run(m, True)
        _, _, g_twice = _run(m, True, clear=False)  # gradients already there: the second backward adds to them
    finally:
        m._grad_bucket_hook, m.grad_bucket_blocks = None, 0
    assert seen[:2] == [(1, 3, (2, 4, 64, 1920), (2, 4, 1920, 64)), (0, 1, (1, 4, 64, 1920), (1, 4, 1920, 64))] and seen[2:] == seen[:2]
    e1, e2 = _rel(g_rng, g_one), _rel(g_twice, 2 * g_rng)
    print(f"[cog-ckpt ranges] (1, 3) + (0, 1) vs one range {e1:.3e}; second backward vs twice {e2:.3e}")
    assert e1 < 1e-6 and e2 < 1e-5


@pytest.mark.parametrize("r", [64, 0])
def test_c_abi_recompute_leaves_the_callers_output_alone(r):
    """ftmi_cog_blocks_forward / _backward called directly with checkpoint 0 and 1 over a workspace that starts as NaN bit patterns: the same output and
    the same d_tokens_in bit for bit; a sentinel written into tokens_out between the two calls is still there after the backward (the recomputation of
    block L - 1 stops before the launch that would write it).  r = 0: no adapters, grad_a = grad_b = NULL."""
    from finetrainers_amd import _lib
    from finetrainers_amd.cogvideox.model import rotary_tables

    m, _ = _model(3, True)
    dev = _dev()
    lib = _lib.load()
    B, N, D, L = 2, 88, 1920, 3
    g = torch.Generator().manual_seed(9)
    tokens = torch.randn(B, N, D, generator=g).to(bf16).to(dev)
    temb = torch.nn.functional.silu(torch.randn(B, 512, generator=g)).to(bf16).to(dev)
    dout = (0.01 * torch.randn(B, N, D, generator=g)).to(bf16).to(dev)
    rope = tuple(t.to(dev).float().contiguous() for t in rotary_tables(m.config, 8, 12, 3))
    w = m._c_weights(rope)
    if r == 0:
        for k in ("lora_a_sp", "lora_bt_sp", "lora_b_ext", "lora_at_ext", "lora_at_qkv_ext"):
            setattr(w, k, None)
    sentinel = -7.0
    got = {}
    for ckpt in (0, 1):
        cfg = m._c_config(B, N)
        cfg.checkpoint = ckpt
        if r == 0:
            cfg.r, cfg.lora_scale = 0, 0.0
        nbytes = lib.ftmi_cog_workspace_bytes(ctypes.byref(cfg))
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        out, din = torch.empty_like(tokens), torch.zeros_like(tokens)
        ga = torch.zeros(L, 4, 64, D, device=dev) if r else None
        gb = torch.zeros(L, 4, D, 64, device=dev) if r else None
        _lib.check(lib.ftmi_cog_blocks_forward(ctypes.byref(cfg), ctypes.byref(w), _lib.ptr(tokens), _lib.ptr(temb), _lib.ptr(out), _lib.ptr(ws), nbytes,
                                               _lib.stream_ptr()), "ftmi_cog_blocks_forward")
        kept = out.clone()
        out.fill_(sentinel)
        _lib.check(lib.ftmi_cog_blocks_backward(ctypes.byref(cfg), ctypes.byref(w), _lib.ptr(tokens), _lib.ptr(dout), _lib.ptr(din), _lib.ptr(ga), _lib.ptr(gb),
                                                _lib.ptr(ws), nbytes, L, 0, 0, _lib.stream_ptr()), "ftmi_cog_blocks_backward")
        torch.cuda.synchronize()
        assert bool((out == sentinel).all()), "the backward wrote the caller's tokens_out"
        assert torch.isfinite(kept.float()).all() and torch.isfinite(din.float()).all() and din.float().norm().item() > 0
        got[ckpt] = (kept, din, ga, gb, nbytes)
    assert got[1][4] < got[0][4]
    assert torch.equal(got[1][0], got[0][0]), "tokens_out"
    assert torch.equal(got[1][1], got[0][1]), "d_tokens_in"
    if r:
        ea, eb = _rel(got[1][2], got[0][2]), _rel(got[1][3], got[0][3])
        print(f"[cog-ckpt abi] grad_a {ea:.3e} grad_b {eb:.3e}")
        assert ea < 1e-6 and eb < 1e-6


@pytest.mark.parametrize("rotary", [False, "1.5"])
def test_checkpointed_model_step_parity_two_blocks(rotary):
    """The body of test_gpu_cogvideox.py::test_model_step_parity_two_blocks with the flag on, same bounds (computed from the oracle in this run): the whole
    SFT forward + backward at 2 blocks against oracle/cogvideox.py, then one fused optimisation step."""
    from finetrainers_amd.cogvideox import MI355XCogVideoXSFTStep, MI355XCogVideoXSpecOps
    from oracle import cogvideox as cvx
    from oracle import ltx

    layers = 2
    dev = _dev()
    gmodel, omodel = _model(layers, rotary)
    g = torch.Generator().manual_seed(11)
    B, F_, C, H, W = 2, 3, 16, 8, 12
    lat = torch.randn(B, F_, C, H, W, generator=g).to(bf16)
    F_pad = F_ + (2 - F_ % 2) if rotary == "1.5" else F_  # the specification pads the latent frames to a multiple of patch_size_t before the noise is drawn
    noise = torch.randn(B, F_pad, C, H, W, generator=g).to(bf16)
    text = torch.randn(B, 16, 4096, generator=g).to(bf16)
    sig = torch.tensor([0.21, 0.77])
    osch = cvx.CogVideoXDDIMScheduler()

    def run_oracle(model=omodel, cast=bf16):
        for p in model.parameters():
            p.grad = None
        pred, target, _ = cvx.spec_forward(model, osch, lat.to(cast), text.to(cast), sig, noise=noise.to(cast))
        loss = cvx.sft_loss(pred, target, sig, osch)
        loss.backward()
        return loss.item(), pred.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    loss_ref, pred_ref, g_ref = run_oracle()
    with ltx.accumulation_order_variant(512):
        _, _, g_alt = run_oracle()
    floor, floor_worst = ltx.grads_rel_l2(g_alt, g_ref)
    _, _, g32 = run_oracle(copy.deepcopy(omodel).float(), torch.float32)
    o32, o32_worst = ltx.grads_rel_l2(g_ref, g32)

    before = gmodel.lora_flat.clone()
    gmodel.enable_gradient_checkpointing()
    try:
        assert gmodel.native_blocks and gmodel.is_gradient_checkpointing
        for blk in gmodel.transformer_blocks:
            blk.lora_A.grad = blk.lora_B.grad = None
        spec = MI355XCogVideoXSpecOps()
        pred, target, _ = spec.forward(gmodel, lat.to(dev), text.to(dev), sig.to(dev), noise=noise.to(dev))
        loss = spec.loss_backward(pred, target, sig.to(dev))
        torch.cuda.synchronize()
        got = {}
        for i, blk in enumerate(gmodel.transformer_blocks):
            for j, n in enumerate(("to_q", "to_k", "to_v", "to_out.0")):
                got[f"transformer_blocks.{i}.attn1.{n}.lora_A.default.weight"] = blk.lora_A.grad[j].cpu()
                got[f"transformer_blocks.{i}.attn1.{n}.lora_B.default.weight"] = blk.lora_B.grad[j].cpu()
        assert set(got) == set(g_ref)
        glob, worst = ltx.grads_rel_l2(got, g_ref)
        e_pred, e_loss = _rel(pred.cpu(), pred_ref), abs(loss.item() - loss_ref) / abs(loss_ref)
        print(f"[cog-ckpt model L={layers} rotary={rotary}] pred {e_pred:.2e} loss {loss.item():.6f} vs {loss_ref:.6f} (rel {e_loss:.2e}) | LoRA grads {glob:.2e} "
              f"(worst {worst:.2e}); summation-order floor {floor:.2e} / {floor_worst:.2e}")
        assert e_pred < 1e-2 * max(1.0, layers / 8) and e_loss < 1e-3
        assert glob < 2.5 * floor + 1e-3 and worst < 2.5 * floor_worst + 2e-3
        k32, k32_worst = ltx.grads_rel_l2(got, g32)
        print(f"[cog-ckpt model L={layers} rotary={rotary}] vs the fp32 evaluation of the graph: kernel {k32:.2e} / {k32_worst:.2e}, bf16 oracle {o32:.2e} / {o32_worst:.2e}")
        assert k32 < 1.15 * o32 + 3e-4 and k32_worst < 1.3 * o32_worst + 1e-3

        for blk in gmodel.transformer_blocks:
            blk.lora_A.grad = blk.lora_B.grad = None
        step = MI355XCogVideoXSFTStep(gmodel, spec, lr=1e-3, betas=(0.9, 0.99), generator=torch.Generator(device=dev).manual_seed(3))
        out = step.step(lat.to(dev), text.to(dev), sigmas=sig.to(dev), noise=noise.to(dev))
        torch.cuda.synchronize()
        gn_ref = math.sqrt(sum(float(v.double().pow(2).sum()) for v in g_ref.values()))
        print(f"[cog-ckpt step] loss {out['loss'].item():.6f} grad_norm {out['grad_norm'].item():.5e} vs oracle {gn_ref:.5e}")
        assert abs(out["loss"].item() - loss_ref) < 1e-3 * abs(loss_ref) and abs(out["grad_norm"].item() - gn_ref) < 5e-3 * gn_ref
        assert not torch.equal(gmodel.lora_flat, before) and gmodel.transformer_blocks[0].lora_A.grad is None
    finally:
        gmodel.disable_gradient_checkpointing()
        with torch.no_grad():  # the model is shared: the adapters go back to what they were
            gmodel.lora_flat.copy_(before)
        gmodel._lora_versions = None


def test_peak_memory_drops_by_the_slots_that_are_gone():
    """3 layers: three block slots become one.  blk_stride comes from the library's own plan: kept - checkpointed = 2 slots (to the allocator's 256 bytes)."""
    from finetrainers_amd import _lib

    m, _ = _model(3, True)
    lib = _lib.load()
    plan = {}
    for ckpt in (0, 1):
        cfg = m._c_config(2, 88)
        cfg.checkpoint = ckpt
        plan[ckpt] = lib.ftmi_cog_workspace_bytes(ctypes.byref(cfg))
    blk_stride = (plan[0] - plan[1]) / 2
    assert blk_stride > 0
    peak = {}
    for ckpt in (False, True):
        m._ws_pool.clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        _run(m, ckpt)
        peak[ckpt] = torch.cuda.max_memory_allocated()
    m._ws_pool.clear()
    print(f"[cog-ckpt memory] peak {peak[False] / 2**20:.1f} MiB kept, {peak[True] / 2**20:.1f} MiB checkpointed; block slot {blk_stride / 2**20:.1f} MiB, "
          f"planned workspace {plan[0] / 2**20:.1f} -> {plan[1] / 2**20:.1f} MiB")
    assert peak[False] - peak[True] >= 1.5 * blk_stride
