"""Wan image-to-video LoRA, the parts that need no GPU: the byte planners of ``ftmi_wan_lora_ffn_block_*`` with an image context, the width limit, the unchanged T2V plans, the
diffusers I2V state-dict names, the adapter set on an I2V model and the 36-channel input the specification builds."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE_REGEX = "blocks.*(to_q|to_k|to_v|to_out.0)"  # examples/training/sft/wan_i2v/3dgs_dissolve/train.sh --target_modules
NEW_SYMBOLS = ("ftmi_attn_ctx2_fwd", "ftmi_attn_ctx2_dq")
GEOMS = [(2, 48, 16, 256, 2, 512), (1, 200, 64, 1536, 12, 8960), (1, 136, 16, 5120, 40, 13824)]  # B, S, T, D, H, F
KW = dict(num_attention_heads=2, attention_head_dim=128, ffn_dim=512, text_dim=64, image_dim=128, in_channels=36)
bf16 = torch.bfloat16


def _cfg(B, S, T, D, H, F, r, TI):
    import wan_lora_bytes

    return wan_lora_bytes.config(B, S, T, D, H, F, r, TI)


def _last_error(lib):
    buf = ctypes.create_string_buffer(512)
    lib.ftmi_last_error(buf, 512)
    return buf.value.decode()


def test_c_abi_exports_and_declares_the_i2v_entries():
    """The image attention's two kernels and the one LoRA block family that takes the image context; the narrow families' names are gone."""
    import wan_lora_bytes
    from finetrainers_amd import _lib

    lib = _lib.load()
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "ftmi355.h")).read()))
    for name in NEW_SYMBOLS:
        assert name in declared and getattr(lib, name) is not None, name
    wan_lora_bytes.assert_only_the_wide_family(lib, declared, set(_lib.EXPORTED_SYMBOLS))


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("r", [0, 64, 128])
def test_i2v_planners_are_consistent_and_grow_with_the_image_tokens(geom, r):
    """TI = 0: the T2V LoRA plan as recorded (tests/golden/wan_lora_entry_bytes.txt), byte for byte.  TI > 0: saved grows by exactly the four image buffers
    (each rounded to 256 bytes like every entry of the plan), monotonically in TI, and lands on the recorded bytes at TI = 257 and 320; the scratch plan does
    not depend on TI."""
    import wan_lora_bytes
    from finetrainers_amd import _lib

    lib = _lib.load()
    B, S, T, D, H, F = geom
    plans = wan_lora_bytes.recorded()
    saved0, scratch0 = plans[(B, S, T, D, H, F, r, 0, 0)]
    assert saved0 > 0 and scratch0 > 0
    up = lambda n: (n + 255) // 256 * 256
    prev = saved0
    for TI in (0, 1, 64, 257, 320):
        saved, scratch = wan_lora_bytes.planned(B, S, T, D, H, F, r, TI)
        want = saved0 if TI == 0 else saved0 + up(B * TI * 2 * D * 2) + up(B * TI * D * 2) + up(B * H * S * 4) + up(B * S * D * 2)
        assert saved == want and scratch == scratch0, (TI, saved, want, scratch, scratch0)
        assert saved >= prev and (TI == 0 or saved > saved0)
        if TI in (0, 257, 320):
            assert (saved, scratch) == plans[(B, S, T, D, H, F, r, TI, 0)]
        prev = saved
    assert lib.ftmi_wan_lora_ffn_block_saved_bytes(ctypes.byref(_cfg(B, S, T, D, H, F, r, 321))) == 0 and "320" in _last_error(lib)
    assert plans[(B, S, T, D, H, F, r, 321, 0)] == (0, 0)


def test_width_5120_is_accepted_and_5184_refused():
    """Through the planner and through the forward entry (which checks the configuration before it touches a pointer: the 5120 call gets as far as the
    buffer-size check, the 5184 call is refused with the limit in its message)."""
    import wan_lora_bytes
    from finetrainers_amd import _lib

    lib = _lib.load()
    ok, bad = _cfg(1, 136, 16, 5120, 40, 13824, 64, 257), _cfg(1, 136, 16, 5184, 40, 13824, 64, 257)
    bad.H = 5184 // 128  # 40.5 heads do not exist: give it a width that is heads x 128 + 64 either way
    assert lib.ftmi_wan_lora_ffn_block_saved_bytes(ctypes.byref(ok)) > 0
    assert lib.ftmi_wan_lora_ffn_block_saved_bytes(ctypes.byref(bad)) == 0 and "5120" in _last_error(lib)
    wide = _cfg(1, 136, 16, 5248, 41, 13824, 64, 257)  # a whole number of heads, past the limit
    assert lib.ftmi_wan_lora_ffn_block_saved_bytes(ctypes.byref(wide)) == 0 and "at most 5120" in _last_error(lib)
    w = _lib.WanLoraFfnBlockWeights()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    w.base.params = p
    for cfg, msg in ((ok, "buffer too small"), (bad, "at most 5120"), (wide, "at most 5120")):
        rc = lib.ftmi_wan_lora_ffn_block_forward(ctypes.byref(cfg), ctypes.byref(w), p, p, p, p, p, p, p, p, p, 0, p, 0, None)
        assert rc != 0 and msg in _last_error(lib), (cfg.D, rc, _last_error(lib))
    plans = wan_lora_bytes.recorded()  # the widest geometry's plans, with and without the image tokens, are the recorded ones
    for TI in (0, 257):
        assert wan_lora_bytes.planned(1, 136, 16, 5120, 40, 13824, 64, TI) == plans[(1, 136, 16, 5120, 40, 13824, 64, TI, 0)] > (0, 0)
    assert plans[(1, 136, 16, 5184, 40, 13824, 64, 257, 0)] == plans[(1, 136, 16, 5248, 41, 13824, 64, 257, 0)] == (0, 0)


def test_recorded_t2v_plans_have_not_moved():
    """tests/golden/wan_block_bytes.txt: the full fine-tune's columns through its planners, the LoRA columns through the one LoRA entry at TI = 0, ffn = 0 --
    which tests/golden/wan_lora_entry_bytes.txt records as well, with the same numbers."""
    import wan_lora_bytes
    from finetrainers_amd import _lib

    lib = _lib.load()
    rows = [ln.split() for ln in open(os.path.join(ROOT, "tests", "golden", "wan_block_bytes.txt")) if ln.strip() and not ln.startswith("#")]
    assert len(rows) == 18
    plans = wan_lora_bytes.recorded()
    for row in rows:
        B, S, T, D, H, F, r, full_saved, full_scratch, elements, lora_saved, lora_scratch = map(int, row)
        full = ctypes.byref(_lib.WanBlockConfig(B=B, S=S, T=T, D=D, H=H, F=F, eps=1e-6, gemm_variant=8))
        got = (lib.ftmi_wan_block_saved_bytes(full), lib.ftmi_wan_block_scratch_bytes(full), lib.ftmi_wan_block_param_elements(full)) + \
            wan_lora_bytes.planned(B, S, T, D, H, F, r, 0)
        assert got == (full_saved, full_scratch, elements, lora_saved, lora_scratch), (row, got)
        assert plans[(B, S, T, D, H, F, r, 0, 0)] == (lora_saved, lora_scratch)


def _pair(layers=2):
    import wan_i2v_reference as ref
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig

    torch.manual_seed(0)
    kw = {k: v for k, v in KW.items() if k != "in_channels"}
    omodel = ref.WanI2VTransformer3DModel(ref.WanI2VConfig(num_layers=layers, **kw)).to(bf16)
    return omodel, MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, **KW), device=torch.device("cpu"))


def _fix(k):
    return k.replace("ffn.proj_in.", "ffn.net.0.proj.").replace("ffn.proj_out.", "ffn.net.2.")


def test_state_dict_round_trip_with_the_diffusers_i2v_names():
    omodel, model = _pair()
    sd = {_fix(k): v for k, v in omodel.state_dict().items()}
    for name in ("condition_embedder.image_embedder.norm1.weight", "condition_embedder.image_embedder.ff.net.0.proj.bias",
                 "condition_embedder.image_embedder.ff.net.2.weight", "condition_embedder.image_embedder.norm2.bias", "blocks.1.attn2.add_k_proj.weight",
                 "blocks.0.attn2.add_v_proj.bias", "blocks.1.attn2.norm_added_k.weight"):
        assert name in sd, name  # the names diffusers gives these modules
    model.load_diffusers_state_dict(sd)
    views = model.state_dict_views()
    assert set(views) == set(sd)
    for k, v in sd.items():
        assert torch.equal(views[k].reshape(-1), v.reshape(-1)), k
    assert tuple(views["patch_embedding.weight"].shape) == (256, 36 * 4)  # 16 noised + 4 mask + 16 conditioning channels x (1, 2, 2)
    with pytest.raises(KeyError, match="add_"):
        model.blocks[0].load_diffusers_state_dict({k[len("blocks.0."):]: v for k, v in sd.items() if k.startswith("blocks.0.") and "add_k_proj" not in k})


def test_i2v_adapters_are_the_eight_attention_projections():
    omodel, model = _pair()
    model.add_adapter(32, 32.0, target_modules=RECIPE_REGEX)
    targets = [n for n, _ in omodel.named_modules() if re.fullmatch(RECIPE_REGEX, n)]  # peft: fullmatch against every module name
    assert len(targets) == 16 and not any("add_" in n for n in targets)
    sd = model.lora_state_dict()
    assert set(sd) == {f"{n}.lora_{ab}.weight" for n in targets for ab in "AB"}
    assert not any("add_k_proj" in k or "add_v_proj" in k for k in sd)
    assert all(blk.lora_A.shape[0] == 8 for blk in model.blocks) and len(model.lora_parameters()) == 4
    assert not any(blk.img_flat.requires_grad or blk.flat.requires_grad for blk in model.blocks)


def test_model_refuses_what_is_out_of_scope():
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig

    _, model = _pair(1)
    x, t, text, img = torch.zeros(1, 36, 2, 8, 12), torch.zeros(1), torch.zeros(1, 16, 64), torch.zeros(1, 257, 128)
    with pytest.raises(NotImplementedError, match="full fine-tuning"):
        model(x, t, text, encoder_hidden_states_image=img)
    with pytest.raises(NotImplementedError, match="image"):
        model(x, t, text)
    t2v = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=1, **{k: v for k, v in KW.items() if k not in ("image_dim", "in_channels")}),
                                      device=torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="image"):
        t2v(torch.zeros(1, 16, 2, 8, 12), t, text, encoder_hidden_states_image=img)


def test_specification_builds_the_36_channel_input_in_the_reference_order(monkeypatch):
    """``MI355XWanModelSpecification.forward`` up to the model call against the torch restatement of base_specification.py:457-481 on CPU tensors: channels
    [noisy 16 | mask 4 | condition 16], the condition = the normalised MEAN of its moments (the posterior's mode), the image embeddings passed on."""
    import wan_i2v_reference as ref
    from finetrainers_amd import ops
    from finetrainers_amd.wan import MI355XWanModelSpecification
    from oracle import wan

    g = torch.Generator().manual_seed(3)
    B, C, F_, H, W = 2, 16, 2, 8, 12
    mom = lambda: torch.cat([torch.randn(B, C, F_, H, W, generator=g), 0.3 * torch.randn(B, C, F_, H, W, generator=g) - 2.0], dim=1).to(bf16)
    moments, cond, mask = mom(), mom(), (torch.rand(B, 4, F_, H, W, generator=g) < 0.3).to(bf16)
    eps, noise = (torch.randn(B, C, F_, H, W, generator=g).to(bf16) for _ in range(2))
    mean, std, sigmas = 0.1 * torch.randn(C, generator=g), 1.0 + 0.2 * torch.rand(C, generator=g), torch.tensor([0.23, 0.81])
    text, image = torch.randn(B, 16, 64, generator=g).to(bf16), torch.randn(B, 257, 128, generator=g).to(bf16)
    # the posterior draw is a library kernel on the GPU: its arithmetic on CPU tensors, for this host test
    monkeypatch.setattr(ops, "posterior_sample", lambda m, e: wan.posterior_sample(m, e))
    seen = {}

    def transformer(**kw):
        seen.update(kw)
        return (torch.zeros(B, C, F_, H, W, dtype=bf16),)

    spec = MI355XWanModelSpecification(pretrained_model_name_or_path=None)
    latent = {"latents": moments, "latents_mean": mean, "latents_std": std, "latent_condition": cond, "latent_condition_mask": mask}
    _, target, _ = spec.forward(transformer, {"encoder_hidden_states": text, "encoder_hidden_states_image": image}, latent, sigmas, posterior_noise=eps, noise=noise)
    hidden, latents, timesteps = ref.i2v_model_input(moments, mean, std, sigmas.view(-1, 1, 1, 1, 1), eps, noise, cond, mask)
    assert tuple(seen["hidden_states"].shape) == (B, 36, F_, H, W) and seen["hidden_states"].dtype == bf16
    assert torch.equal(seen["hidden_states"], hidden) and torch.equal(seen["timestep"], timesteps) and torch.equal(target, noise - latents)
    assert torch.equal(seen["hidden_states"][:, 16:20], mask) and torch.equal(seen["hidden_states"][:, 20:], wan.normalize_latents(cond[:, :C], mean, std))
    assert seen["encoder_hidden_states_image"] is image and seen["encoder_hidden_states"] is text
    with pytest.raises(ValueError, match="together"):
        spec.forward(transformer, {"encoder_hidden_states": text}, {"latents": moments, "latents_mean": mean, "latents_std": std, "latent_condition": cond}, sigmas)
