"""Wan first/last-frame image-to-video LoRA (a config with ``pos_embed_seq_len``), the parts that need no GPU: the two wide second-context entries and their
refusals, the byte planners of ``ftmi_wan_lora_ffn_block_*`` with a second image (TI2), the configuration key, ``pos_embed`` in the state dict, the image embedder
against tests/wan_flf_reference.py and the conditioning mask."""
import ctypes
import os
import re

import pytest
import torch

import test_attention_refusals_host as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ftmi_attn_ctx2w_fwd", "ftmi_attn_ctx2w_dq")
GEOMS = [(2, 48, 16, 256, 2, 512), (1, 200, 64, 1536, 12, 8960), (1, 136, 16, 5120, 40, 13824)]  # B, S, T, D, H, F
KW = dict(num_attention_heads=2, attention_head_dim=128, ffn_dim=512, text_dim=64, image_dim=128, in_channels=36)
bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    from finetrainers_amd import _lib

    return _lib.load()


def _cfg(B, S, T, D, H, F, r, TI, TI2, ffn=0):
    from finetrainers_amd import _lib

    return _lib.WanLoraFfnBlockConfig(B=B, S=S, T=T, D=D, H=H, F=F, eps=1e-6, gemm_variant=8, r=r, lora_scale=1.0, TI=TI, ffn=ffn, TI2=TI2)


def _planned(lib, *a, **kw):
    c = ctypes.byref(_cfg(*a, **kw))
    return lib.ftmi_wan_lora_ffn_block_saved_bytes(c), lib.ftmi_wan_lora_ffn_block_scratch_bytes(c)


def test_c_abi_gains_exactly_the_two_wide_entries_and_keeps_its_version(lib):
    from finetrainers_amd import _lib

    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    product = re.sub(r"#ifdef FTMI_EXPERIMENTAL.*?#endif", "", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S)
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", product))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
    assert {n for n in declared if "ctx2" in n} == {"ftmi_attn_ctx2_fwd", "ftmi_attn_ctx2_dq"} | set(NEW_SYMBOLS)
    assert lib.ftmi_version() == 101
    # both structures grew by one trailing int, in the header and in the Python mirror
    for struct, c_name in ((_lib.WanLoraFfnBlockConfig, "ftmi_wan_lora_ffn_block_config"), (_lib.WanSampleConfig, "ftmi_wan_sample_config")):
        assert struct._fields_[-1] == ("TI2", ctypes.c_int)
        assert struct.TI2.offset == ctypes.sizeof(struct) - ctypes.sizeof(ctypes.c_int)
        body = re.search(r"typedef struct[^{}]*\{([^{}]*)\}\s*" + c_name + ";", product).group(1)
        assert [s.strip() for s in body.split(";") if s.strip()][-1] == "int TI2"


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("r,ffn", [(0, 0), (64, 0), (128, 1)])
def test_planners_grow_by_the_second_images_rows_alone(lib, geom, r, ffn):
    """TI = 257: with TI2 = 0 the plan is the recorded single-image one; TI2 > 0 grows ``saved`` by kvi [B TI2, 2D] and kin [B TI2, D] and by nothing else (each
    entry of the plan rounded to 256 bytes); ``scratch`` does not move."""
    import wan_lora_bytes

    B, S, T, D, H, F = geom
    TI = 257
    saved0, scratch0 = _planned(lib, B, S, T, D, H, F, r, TI, 0, ffn)
    assert (saved0, scratch0) == wan_lora_bytes.recorded()[(B, S, T, D, H, F, r, TI, ffn)] > (0, 0)
    up = lambda n: (n + 255) // 256 * 256
    for TI2 in (0, 1, 257, 320):
        saved, scratch = _planned(lib, B, S, T, D, H, F, r, TI, TI2, ffn)
        grow = up(B * (TI + TI2) * 2 * D * 2) - up(B * TI * 2 * D * 2) + up(B * (TI + TI2) * D * 2) - up(B * TI * D * 2)
        assert saved == saved0 + grow and scratch == scratch0, (TI2, saved, saved0, grow, scratch, scratch0)
        assert TI2 == 0 or saved > saved0


def test_planner_refusals(lib):
    g = (2, 48, 16, 256, 2, 512, 64)
    assert _planned(lib, *g, 257, 321) == (0, 0) and "second image" in ar.last_error(lib) and "320" in ar.last_error(lib)
    assert _planned(lib, *g, 257, -1) == (0, 0) and "second image" in ar.last_error(lib)
    assert _planned(lib, *g, 0, 257) == (0, 0) and "TI > 0" in ar.last_error(lib)
    assert _planned(lib, *g, 321, 0) == (0, 0) and "0 .. 320" in ar.last_error(lib)
    assert _planned(lib, *g, 321, 257) == (0, 0) and "the image context holds 0 .. 320 tokens" in ar.last_error(lib)
    assert _planned(lib, *g, 320, 320) > (0, 0)
    # the sampler's planner hands TI2 to the block's
    from finetrainers_amd import _lib, ops

    geo = ops.wan_sample_geometry(1, 16, 2, 8, 12, 192, extra_channels=20, copies=1, guidance=True)
    base = dict(geo=geo, T=16, D=256, heads=2, ffn_dim=512, L=2, eps=1e-6, gemm_variant=8, r=64, lora_scale=1.0, ffn=0, patch_fold=0, patch_r=0, patch_scale=0.0,
                steps=2, guidance=5.0)
    ws = lambda **kw: lib.ftmi_wan_sample_workspace_bytes(ctypes.byref(_lib.WanSampleConfig(**base, **kw)))
    one, two = ws(TI=257, TI2=0), ws(TI=257, TI2=257)
    up = lambda n: (n + 255) // 256 * 256
    assert one > 0 and two - one == up(2 * 514 * 512 * 2) - up(2 * 257 * 512 * 2) + up(2 * 514 * 256 * 2) - up(2 * 257 * 256 * 2)
    assert ws(TI=257, TI2=321) == 0 and "second image" in ar.last_error(lib)
    assert ws(TI=0, TI2=257) == 0


def _wfwd(lib, t, ptrs=None):
    p = dict(q=ar.BASE, k=ar.BASE + 16, v=ar.BASE + 32, out_first=ar.BASE + 48, out=ar.BASE + 64, lse=ar.BASE + 80)
    p.update(ptrs or {})
    return lib.ftmi_attn_ctx2w_fwd(ctypes.byref(t) if t is not None else None, p["q"], p["k"], p["v"], p["out_first"], p["out"], p["lse"], None)


def _wdq(lib, t, ptrs=None):
    p = dict(q=ar.BASE, k=ar.BASE + 16, v=ar.BASE + 32, lse=ar.BASE + 48, dout=ar.BASE + 64, dq_first=ar.BASE + 80, dq=ar.BASE + 96)
    p.update(ptrs or {})
    return lib.ftmi_attn_ctx2w_dq(ctypes.byref(t) if t is not None else None, p["q"], p["k"], p["v"], p["lse"], p["dout"], p["dq_first"], p["dq"], None)


@pytest.mark.parametrize("which", ["fwd", "dq"])
def test_wide_kernel_refusals_carry_the_narrow_pairs_codes(lib, which):
    """Every call returns before a launch: the pointers are host addresses that are never read."""
    call, narrow = (_wfwd, ar.c2fwd) if which == "fwd" else (_wdq, ar.c2dq)
    desc, refused = ar.desc, ar.refused
    refused(lib, call(lib, None), ar.INVALID, "null descriptor")
    refused(lib, call(lib, desc(d=64)), ar.UNSUPPORTED, "attn_ctx2w", "head_dim must be 128")
    for field, val in (("Sk", 0), ("Sk", -1), ("H", 0), ("B", -1), ("Sq", -1)):
        t = desc(d=128)
        setattr(t, field, val)
        refused(lib, call(lib, t), ar.INVALID, "attn_ctx2w", "empty key set or negative size")
    refused(lib, call(lib, desc(d=128, Sk=641)), ar.UNSUPPORTED, "attn_ctx2w", "at most 640 keys")
    refused(lib, call(lib, desc(d=128, Sk=2**31 - 1)), ar.UNSUPPORTED, "640")
    for Sk in (321, 514, 640):  # accepted as far as the next check
        refused(lib, call(lib, desc(d=128, Sk=Sk), {"q": None}), ar.INVALID, f"ftmi_attn_ctx2w_{which}: null tensor")
    names = ("q", "k", "v", "out_first", "out", "lse") if which == "fwd" else ("q", "k", "v", "lse", "dout", "dq_first", "dq")
    for name in names:
        refused(lib, call(lib, desc(d=128, Sk=514), {name: None}), ar.INVALID, f"ftmi_attn_ctx2w_{which}: null tensor")
    groups = [(("q", "k", "v"), "q / k / v rows")] + ([(("out",), "output rows")] if which == "fwd" else [(("dout", "dq"), "dO / dQ rows")])
    for tensors, word in groups:
        for tn in tensors:
            for axis in range(3):
                t = desc(d=128, Sk=514)
                getattr(t, ar.STRIDES_OF[tn])[axis] += 4
                refused(lib, call(lib, t), ar.INVALID, "attn_ctx2w", word, "16-byte alignment")
            refused(lib, call(lib, desc(d=128, Sk=514), {tn: ar.BASE + 8}), ar.INVALID, "attn_ctx2w", word, "16-byte alignment")
    refused(lib, call(lib, desc(d=128, Sk=514), {"out_first" if which == "fwd" else "dq_first": ar.BASE + 8}), ar.INVALID, "16-byte alignment")
    assert call(lib, desc(d=128, B=0, Sk=514)) == 0 and call(lib, desc(d=128, Sq=0, Sk=514)) == 0
    # the narrow pair keeps its limit and its message
    refused(lib, narrow(lib, desc(d=128, Sk=321)), ar.UNSUPPORTED, "attn_ctx2:", "at most 320 keys")
    refused(lib, narrow(lib, desc(d=128, Sk=320), {"q": None}), ar.INVALID, "null tensor")


# ---- configuration, parameters, image embedder ------------------------------------------------------------------------------------------------------------------
def test_config_keeps_and_checks_pos_embed_seq_len():
    from finetrainers_amd.wan import WanTransformerConfig

    disk = dict(KW, num_layers=2, pos_embed_seq_len=514, _class_name="WanTransformer3DModel", added_kv_proj_dim=256)
    cfg = WanTransformerConfig.from_dict(disk)
    assert cfg.pos_embed_seq_len == 514 and cfg.second_image_tokens == 257
    plain = WanTransformerConfig.from_dict({k: v for k, v in disk.items() if k != "pos_embed_seq_len"})
    assert plain.pos_embed_seq_len is None and plain.second_image_tokens == 0
    assert WanTransformerConfig.from_dict(dict(disk, pos_embed_seq_len=None)).pos_embed_seq_len is None
    assert WanTransformerConfig.from_dict(dict(disk, pos_embed_seq_len=640)).second_image_tokens == 320
    with pytest.raises(ValueError, match="even"):
        WanTransformerConfig.from_dict(dict(disk, pos_embed_seq_len=513))
    with pytest.raises(ValueError, match="640"):
        WanTransformerConfig.from_dict(dict(disk, pos_embed_seq_len=642))
    with pytest.raises(ValueError, match="image_dim"):
        WanTransformerConfig.from_dict({k: v for k, v in disk.items() if k != "image_dim"})
    with pytest.raises(ValueError):
        WanTransformerConfig.from_dict(dict(disk, pos_embed_seq_len=0))


def _pair(layers=1, n_pos=514, seed=0):
    import wan_flf_reference as ref
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig

    torch.manual_seed(seed)
    kw = {k: v for k, v in KW.items() if k != "in_channels"}
    omodel = ref.WanFLFTransformer3DModel(ref.WanFLFConfig(num_layers=layers, pos_embed_seq_len=n_pos, **kw))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        emb = omodel.condition_embedder.image_embedder
        emb.pos_embed.copy_(0.5 * torch.randn(emb.pos_embed.shape, generator=g))
        for n, p in emb.named_parameters():
            if n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif "norm" in n:
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
    omodel = omodel.to(bf16)
    model = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, pos_embed_seq_len=n_pos, **KW), device=torch.device("cpu"))
    return omodel, model


def _fix(k):
    return k.replace("ffn.proj_in.", "ffn.net.0.proj.").replace("ffn.proj_out.", "ffn.net.2.")


def test_state_dict_round_trips_pos_embed_and_the_plain_i2v_keys_stay():
    import test_wan_i2v_host as i2v_host

    omodel, model = _pair()
    sd = {_fix(k): v for k, v in omodel.state_dict().items()}
    name = "condition_embedder.image_embedder.pos_embed"
    assert tuple(sd[name].shape) == (1, 514, 128) and float(sd[name].abs().max()) > 0
    model.load_diffusers_state_dict(sd)
    views = model.state_dict_views()
    assert set(views) == set(sd) and tuple(views[name].shape) == (1, 514, 128)
    for k, v in sd.items():
        assert torch.equal(views[k].reshape(-1), v.reshape(-1)), k
    with pytest.raises(KeyError, match="pos_embed"):
        model.load_diffusers_state_dict({k: v for k, v in sd.items() if k != name})
    # a plain I2V model: the same keys without pos_embed, at the same offsets of the root buffer
    _, plain = i2v_host._pair(1)
    assert set(plain.state_dict_views()) == set(sd) - {name}
    for k, (off, shape) in plain.root_layout.offsets.items():
        assert model.root_layout.offsets[k] == (off, shape), k
    assert model.root_layout.offsets[name][0] == plain.root_layout.total
    assert all(b.second_image_tokens == 257 for b in model.blocks) and all(b.second_image_tokens == 0 for b in plain.blocks)


def test_image_embedder_is_the_references_bit_for_bit_in_both_layouts():
    omodel, model = _pair()
    model.load_diffusers_state_dict({_fix(k): v for k, v in omodel.state_dict().items()})
    g = torch.Generator().manual_seed(5)
    B = 2
    x = torch.randn(B, 514, 128, generator=g).to(bf16)
    with torch.no_grad():
        want = omodel.condition_embedder.image_embedder(x)
        want_pairs = omodel.condition_embedder.image_embedder(x.view(2 * B, 257, 128))
    assert tuple(want.shape) == (B, 514, 256) and torch.equal(want, want_pairs)
    got = model._embed_image(x)
    assert got.dtype == bf16 and tuple(got.shape) == (B, 514, 256) and torch.equal(got, want)
    assert torch.equal(model._embed_image(x.view(2 * B, 257, 128)), want)  # rows 2b, 2b + 1 are sample b's two images
    # pos_embed is added in bf16 before the first norm: without it the result differs
    model.rparam("condition_embedder.image_embedder.pos_embed").zero_()
    assert not torch.equal(model._embed_image(x), want)
    for bad in (torch.zeros(2, 257 + 1, 128), torch.zeros(1, 257, 128), torch.zeros(2, 513, 128), torch.zeros(1, 1028, 128)):
        with pytest.raises(ValueError, match=rf"{bad.shape[1]} tokens.*514"):
            model._embed_image(bad.to(bf16))


def test_a_model_without_the_key_keeps_its_refusal_above_320_tokens():
    import test_wan_i2v_host as i2v_host

    _, plain = i2v_host._pair(1)
    with pytest.raises(NotImplementedError, match="320"):
        plain._embed_image(torch.zeros(1, 514, 128, dtype=bf16))
    assert tuple(plain._embed_image(torch.zeros(1, 320, 128, dtype=bf16)).shape) == (1, 320, 256)


def test_control_and_full_fine_tune_stay_refused():
    _, model = _pair()
    with pytest.raises(NotImplementedError, match="full fine-tuning"):
        model(torch.zeros(1, 36, 2, 8, 12), torch.zeros(1), torch.zeros(1, 16, 64), encoder_hidden_states_image=torch.zeros(1, 514, 128))
    with pytest.raises(NotImplementedError, match="control"):
        model.expand_patch_embedding(52)
    with pytest.raises(NotImplementedError, match="control"):
        model.add_adapter(32, 32.0, target_modules="(^patch_embedding$)|(blocks.*(to_q|to_k|to_v|to_out.0))", rank_pattern={"patch_embedding": 256},
                          alpha_pattern={"patch_embedding": 256})


def test_sampler_arguments_split_the_image_tokens():
    """``c_arguments`` on a CPU model: TI = TI2 = 257 in the sample configuration; any other token count is refused; a plain I2V model passes TI2 = 0."""
    import test_wan_i2v_host as i2v_host
    from finetrainers_amd import ops
    from finetrainers_amd.wan import MI355XWanLatentSampler

    _, model = _pair(2)
    model.add_adapter(32, 32.0)
    sampler = MI355XWanLatentSampler(model)
    geo = sampler.geometry(1, 2, 8, 12, guidance=True)
    cfg, _, keep = sampler.c_arguments(geo, 16, 514, 2, 5.0)
    assert (cfg.TI, cfg.TI2) == (257, 257) and ops.wan_sample_workspace_bytes(cfg) > 0
    with pytest.raises(ValueError, match="514"):
        sampler.c_arguments(geo, 16, 257, 2, 5.0)
    _, plain = i2v_host._pair(2)
    plain.add_adapter(32, 32.0)
    cfg, _, keep = MI355XWanLatentSampler(plain).c_arguments(geo, 16, 257, 2, 5.0)
    assert (cfg.TI, cfg.TI2) == (257, 0)
    g = torch.Generator().manual_seed(1)
    text, cond = torch.zeros(1, 16, 64, dtype=bf16), torch.zeros(1, 20, 2, 8, 12, dtype=bf16)
    for shape in ((1, 257, 128), (2, 514, 128), (1, 514, 64)):
        with pytest.raises(ValueError, match="first/last-frame"):
            sampler.check_inputs(text, text, 5.0, torch.zeros(shape, dtype=bf16), cond, None, 1, 2, 8, 12)
    for shape in ((1, 514, 128), (2, 257, 128)):
        assert sampler.check_inputs(text, text, 5.0, torch.zeros(shape, dtype=bf16), cond, None, 1, 2, 8, 12) is not None


# ---- conditioning mask ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_frames", [1, 5, 81])
@pytest.mark.parametrize("use_last_frame", [False, True])
def test_condition_mask_is_the_processors(num_frames, use_last_frame):
    import wan_flf_reference as ref
    from finetrainers_amd.wan import MI355XWanModelSpecification

    h, w = 4, 6
    F_lat = (num_frames - 1) // 4 + 1
    want = ref.condition_mask(torch.zeros(1, 16, F_lat, h, w), num_frames, use_last_frame)
    got = MI355XWanModelSpecification.condition_mask(num_frames, h, w, use_last_frame)
    assert tuple(got.shape) == (1, 4, F_lat, h, w) and torch.equal(got, want.to(got.dtype))
    # spelled out: latent frame 0 is kept whole; with the last frame, the last latent frame's LAST channel (pixel frame num_frames - 1) as well
    flat = got[0, :, :, 0, 0]
    assert bool((flat[:, 0] == 1).all())
    if num_frames > 1:
        assert flat[:, 1:].sum().item() == (1.0 if use_last_frame else 0.0)
        assert flat[3, -1].item() == (1.0 if use_last_frame else 0.0)
    with pytest.raises(ValueError):
        MI355XWanModelSpecification.condition_mask(6, h, w, use_last_frame)
