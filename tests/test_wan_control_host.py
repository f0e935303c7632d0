"""Wan control LoRA, the parts that need no GPU: the frame-conditioning restatement against fixtures produced by the reference's own function
(tools/make_wan_control_golden.py), which adapter set the control trainer's ``target_modules`` selects (peft's rule, recomputed here), the widened patch
embedding against the reference's conv expansion, state-dict keys and shapes, the adapter file round trip with ``rank_pattern`` / ``alpha_pattern``, the
step object's layout, and what is refused."""
import os
import random
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(num_attention_heads=2, attention_head_dim=128, ffn_dim=512, text_dim=64)
D, F = 256, 512
RECIPE = "blocks.*(to_q|to_k|to_v|to_out.0|ff.net.0.proj|ff.net.2)"  # examples/training/control/wan/image_condition/train.sh
TEN = "blocks.*(to_q|to_k|to_v|to_out.0|ffn.net.0.proj|ffn.net.2)"
PATTERN = {"patch_embedding": D}  # trainer/control_trainer/trainer.py:137-142: rank_pattern = alpha_pattern = {injection layer: its output width}


def _control_target(target_modules):
    """trainer/control_trainer/trainer.py::_get_lora_target_modules."""
    if isinstance(target_modules, list):
        return list(target_modules) + ["^patch_embedding$"]
    return f"(^patch_embedding$)|({target_modules})"


def _module_names(layers):
    ce = "condition_embedder."
    names = ["patch_embedding", ce + "time_embedder.linear_1", ce + "time_embedder.linear_2", ce + "time_proj", ce + "text_embedder.linear_1", ce + "text_embedder.linear_2"]
    for i in range(layers):
        for a in ("attn1", "attn2"):
            names += [f"blocks.{i}.{a}.{t}" for t in ("to_q", "to_k", "to_v", "to_out.0")]
        names += [f"blocks.{i}.ffn.net.0.proj", f"blocks.{i}.ffn.net.2"]
    return names + ["proj_out"]


def _peft_select(target_modules, names):
    if isinstance(target_modules, str):
        return [n for n in names if re.fullmatch(target_modules, n)]
    return [n for n in names if any(n == t or n.endswith("." + t) for t in target_modules)]


def _model(layers=2, in_channels=16, **kw):
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig

    return MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, in_channels=in_channels, **SMALL, **kw), device=torch.device("cpu"))


@pytest.fixture(scope="module")
def fixtures():
    from safetensors.torch import load_file

    return load_file(os.path.join(ROOT, "tests", "golden", "wan_control_fixtures.safetensors"))


def _cases(fixtures):
    for key in sorted(fixtures):
        if key.startswith("fc.") and key.endswith(".out"):
            _, name, n, e, i, s, _ = key.split(".")
            yield key[:-4], name, int(n[1:]), int(e[1:]), (None if i == "iNone" else int(i[1:])), int(s[1:])


def test_frame_conditioning_equals_the_reference_bit_for_bit(fixtures):
    """All five types; control clips shorter than, as long as and longer than the latents; ``prefix`` / ``random`` under three seeds -- same frames, same bits
    (the sign of a zeroed element included), without and with the concatenated mask."""
    from finetrainers_amd.control import apply_frame_conditioning_on_latents

    seen = set()
    for key, name, n, e, index, seed in _cases(fixtures):
        x = fixtures[f"fc.in.n{n}"]
        for suffix, cat in ((".out", False), (".outmask", True)):
            random.seed(seed)
            got = apply_frame_conditioning_on_latents(x.clone(), e, channel_dim=1, frame_dim=2, frame_conditioning_type=name, frame_conditioning_index=index,
                                                      concatenate_mask=cat)
            want = fixtures[key + suffix]
            assert got.shape == want.shape and got.dtype == want.dtype, key + suffix
            assert torch.equal(got.contiguous().view(torch.int16), want.view(torch.int16)), key + suffix
        seen.add((name, n < e, n == e, n > e))
    assert {s[0] for s in seen} == {"index", "prefix", "random", "first_and_last", "full"}
    assert all({(t, True, False, False), (t, False, True, False), (t, False, False, True)} <= seen for t in ("index", "prefix", "random", "first_and_last", "full"))


def test_frame_keep_mask_is_the_mask_the_fixtures_imply(fixtures):
    """The fixture inputs have no zero element, so a frame of the output is non-zero exactly where the reference kept it."""
    from finetrainers_amd.control import frame_keep_mask

    count = 0
    for key, name, n, e, index, seed in _cases(fixtures):
        implied = (fixtures[key + ".out"] != 0).flatten(3).any(-1)[0, 0].to(torch.uint8)
        random.seed(seed)
        got = frame_keep_mask(n, e, name, index)
        assert got.dtype == torch.uint8 and got.shape == (e,) and torch.equal(got, implied), key
        count += 1
    assert count == 3 * (3 + 3 + 3 + 1 + 1)  # per clip length: three index cases, prefix / random under three seeds, first_and_last, full
    with pytest.raises(ValueError):
        frame_keep_mask(3, 3, "middle")


@pytest.mark.parametrize("user,per_block,patch", [(RECIPE, 8, True), (TEN, 10, True), (["to_q", "to_k", "to_v", "to_out.0"], 8, False),
                                                  (["to_q", "to_k", "to_v", "to_out.0", "net.0.proj", "net.2"], 10, False)])
def test_control_target_modules_select_what_peft_selects(user, per_block, patch):
    layers = 2
    target = _control_target(user)
    selected = _peft_select(target, _module_names(layers))
    # the expectation itself, by peft's rule: the regex form adds patch_embedding; the list form's "^patch_embedding$" is a suffix no module name ends with
    assert ("patch_embedding" in selected) == patch and len([n for n in selected if n.startswith("blocks.")]) == per_block * layers == len(selected) - int(patch)
    model = _model(layers)
    model.expand_patch_embedding(32)
    assert sorted(model.select_modules(target)) == sorted(selected)
    model.add_adapter(32, 16.0, target_modules=target, rank_pattern=PATTERN, alpha_pattern=PATTERN)
    assert model.lora_config == {"r": 32, "lora_alpha": 16.0, "target_modules": target, "rank_pattern": PATTERN, "alpha_pattern": PATTERN}
    sd = model.lora_state_dict()
    assert set(sd) == {f"{n}.lora_{ab}.weight" for n in selected for ab in "AB"}
    assert (model.patch_lora_A is not None) == patch and len(model.lora_parameters()) == layers * (6 if per_block == 10 else 2) + 2 * int(patch)
    if patch:
        assert model.patch_lora_scale == 1.0
        assert model.lora_parameters()[0] is model.patch_lora_A and model.lora_parameters()[1] is model.patch_lora_B


@pytest.mark.parametrize("rank_pattern,alpha_pattern", [(None, None), ({"patch_embedding": 128}, {"patch_embedding": 128}), ({"to_q": D}, None),
                                                        ({"patch_embedding": D}, {"patch_embedding": 0})])
def test_patch_embedding_without_a_full_rank_pattern_raises_naming_it(rank_pattern, alpha_pattern):
    model = _model(2)
    model.expand_patch_embedding(32)
    with pytest.raises(NotImplementedError, match="patch_embedding"):
        model.add_adapter(32, 32.0, target_modules=_control_target(RECIPE), rank_pattern=rank_pattern, alpha_pattern=alpha_pattern)
    assert model.lora_config is None and model.patch_lora_A is None and all(blk.lora_A is None for blk in model.blocks)


def test_pattern_lookup_is_pefts():
    """A key equals the module name or matches ``.*\\.key$``; a pattern that reaches a block projection is refused, naming the projection."""
    model = _model(2)
    model.expand_patch_embedding(32)
    assert model.patch_adapter_spec(_control_target(RECIPE), {"patch_embedding": D}, {"patch_embedding": 2 * D}, 32, 32.0) == (D, 2.0)
    assert model.patch_adapter_spec(_control_target(RECIPE), {"embedding": D}, None, 32, 32.0) == (32, 1.0)  # "embedding" is no dotted suffix of the name
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.attn1\.to_q"):
        model.add_adapter(32, 32.0, target_modules=_control_target(RECIPE), rank_pattern={"patch_embedding": D, "to_q": 64}, alpha_pattern=PATTERN)


def test_expand_patch_embedding_against_the_reference_expansion(fixtures):
    """The reference's ``_expand_conv3d_with_zeroed_weights`` on a Conv3d(4 -> 8): our weight is its weight in GEMM shape, bias unchanged, and every other root
    parameter survives the re-layout bit for bit."""
    from finetrainers_amd.wan.model import RootLayout, WanTransformerConfig

    w, b, we, be = (fixtures[k] for k in ("conv.weight", "conv.bias", "conv.expanded.weight", "conv.expanded.bias"))
    assert we.shape == (8, 8, 1, 2, 2) and torch.equal(we[:, :4], w) and float(we[:, 4:].abs().max()) == 0.0 and torch.equal(be, b)
    model = _model(1, in_channels=16)
    g = torch.Generator().manual_seed(3)
    model.root.data.copy_(torch.randn(model.root.numel(), generator=g))
    before = {k: v.clone() for k, v in model.state_dict_views().items()}
    assert before["patch_embedding.weight"].shape == (D, 64)
    model.expand_patch_embedding(32)
    after = model.state_dict_views()
    assert model.config.in_channels == 32 and after["patch_embedding.weight"].shape == (D, 128)
    assert model.root.numel() == RootLayout(WanTransformerConfig(num_layers=1, in_channels=32, **SMALL)).total
    # the same statement as the fixture's, in GEMM shape: old columns first (columns are (c, pt, ph, pw)), new columns zero
    assert torch.equal(after["patch_embedding.weight"][:, :64], before["patch_embedding.weight"]) and float(after["patch_embedding.weight"][:, 64:].abs().max()) == 0.0
    conv_shape = after["patch_embedding.weight"].reshape(D, 32, 1, 2, 2)
    assert torch.equal(conv_shape[:, :16], before["patch_embedding.weight"].reshape(D, 16, 1, 2, 2))
    for k, v in before.items():
        if k != "patch_embedding.weight":
            assert torch.equal(after[k], v), k


def test_expand_patch_embedding_refusals():
    model = _model(1)
    with pytest.raises(ValueError):
        model.expand_patch_embedding(24)  # 96 patch columns: no multiple of 64
    model.add_adapter(32, 32.0)
    with pytest.raises(RuntimeError):
        model.expand_patch_embedding(32)
    with pytest.raises(NotImplementedError):
        _model(1, in_channels=36, image_dim=128).expand_patch_embedding(52)


def test_state_dict_keys_and_shapes_and_the_adapter_file_round_trip(tmp_path):
    from finetrainers_amd import wire
    from finetrainers_amd.wan import MI355XWanControlModelSpecification

    target = _control_target(RECIPE)
    model = _model(2)
    model.expand_patch_embedding(32)
    model.add_adapter(32, 32.0, target_modules=target, rank_pattern=PATTERN, alpha_pattern=PATTERN)
    sd = model.lora_state_dict()
    assert sd["patch_embedding.lora_A.weight"].shape == (D, 32, 1, 2, 2) and sd["patch_embedding.lora_B.weight"].shape == (D, D, 1, 1, 1)
    assert sd["blocks.1.attn2.to_out.0.lora_A.weight"].shape == (32, D) and len(sd) == 2 + 2 * 16
    bound = (1.0 / 128) ** 0.5  # peft initialises a conv adapter's A kaiming-uniform(a = sqrt(5)) over its own fan-in Cin pt ph pw, B zero
    a = sd["patch_embedding.lora_A.weight"]
    assert float(a.abs().max()) <= bound and float(a.abs().max()) > 0.9 * bound and abs(float(a.mean())) < 0.01 * bound * 10
    assert float(sd["patch_embedding.lora_B.weight"].abs().max()) == 0.0
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for v in sd.values():
            v.copy_(torch.randn(v.shape, generator=g))
    spec = MI355XWanControlModelSpecification(pretrained_model_name_or_path=None)
    norm = {"blocks.0.attn1.norm_q.weight": torch.ones(D)}
    spec._save_lora_weights(str(tmp_path), model.lora_state_dict(), norm, None, wire.lora_config_metadata(32, 32.0, target, rank_pattern=PATTERN, alpha_pattern=PATTERN))
    assert os.path.exists(os.path.join(str(tmp_path), "norm_state_dict.safetensors"))
    loaded, cfg = wire.load_lora_weights(os.path.join(str(tmp_path), "pytorch_lora_weights.safetensors"))
    assert cfg == {"r": 32, "lora_alpha": 32.0, "init_lora_weights": True, "target_modules": target, "rank_pattern": PATTERN, "alpha_pattern": PATTERN}
    assert list(cfg)[-2:] == ["rank_pattern", "alpha_pattern"]  # the control trainer's key order
    fresh = _model(2)
    fresh.expand_patch_embedding(32)
    fresh.add_adapter(cfg["r"], cfg["lora_alpha"], cfg["target_modules"], rank_pattern=cfg["rank_pattern"], alpha_pattern=cfg["alpha_pattern"])
    fresh.load_lora_state_dict(loaded)
    assert all(torch.equal(v, sd[k]) for k, v in fresh.lora_state_dict().items()) and set(fresh.lora_state_dict()) == set(sd)
    eight = _model(2)
    eight.add_adapter(32, 32.0)
    with pytest.raises(KeyError):
        eight.load_lora_state_dict(loaded)


def test_step_object_puts_the_patch_adapter_at_the_front():
    """The two new parameters and their gradients take the first span of the flat buffers; the blocks follow; the last bucket of the exchange goes out when the
    patch-embedding gradients are final, and it starts at element 0."""
    from finetrainers_amd.wan import MI355XWanLoRAStep

    class Recording:
        active, world_size, rank = True, 1, 0

        def __init__(self):
            self.slices = []

        def broadcast_(self, t, src=0):
            pass

        def all_reduce_mean_async(self, t):
            self.slices.append((t.data_ptr(), t.numel()))

    model = _model(3)
    model.expand_patch_embedding(32)
    model.add_adapter(32, 32.0, target_modules=_control_target(RECIPE), rank_pattern=PATTERN, alpha_pattern=PATTERN)
    par = Recording()
    step = MI355XWanLoRAStep(model, parallel=par, grad_bucket_blocks=2)
    patch, per_block = D * 128 + D * D, 16 * 64 * D
    assert step.flat.numel() == patch + 3 * per_block and step._patch_span == (0, patch)
    ga, gb = model._patch_grad_views
    assert model.patch_lora_A.data_ptr() == step.flat.data_ptr() and ga.data_ptr() == step.gflat.data_ptr() and gb.data_ptr() == ga.data_ptr() + 4 * D * 128
    assert [step._spans[id(b)] for b in model.blocks] == [(patch + i * per_block, patch + (i + 1) * per_block) for i in range(3)]
    step.gflat.fill_(1.0)
    grads = model.lora_grad_state_dict()
    assert set(grads) == set(model.lora_state_dict()) and all(float(v.min()) == 1.0 for v in grads.values())
    step._begin_exchange(True)
    for blk in reversed(model.blocks):
        blk._backward_done()
    assert step.bucket_log == [(patch + per_block, patch + 3 * per_block)]  # block 0 alone does not close the buffer any more
    model._patch_grad_hook(model)
    step._finish_exchange()
    assert step.bucket_log == [(patch + per_block, patch + 3 * per_block), (0, patch + per_block)]
    assert step.bucket_log[0][1] == step.gflat.numel() and step.bucket_log[-1][0] == 0
    assert par.slices == [(step.gflat.data_ptr() + 4 * lo, hi - lo) for lo, hi in step.bucket_log]
    assert model._patch_grad_hook is None and all(blk._grad_hook is None for blk in model.blocks)


def test_specification_mirrors_the_reference_interface():
    from finetrainers_amd.wan import MI355XWanControlModelSpecification, WanTransformerConfig

    marker = [object()]
    spec = MI355XWanControlModelSpecification(pretrained_model_name_or_path=None, control_model_processors=marker, transformer_config=WanTransformerConfig(num_layers=1, **SMALL))
    assert spec.control_model_processors is marker and spec.control_injection_layer_name == "patch_embedding"
    assert spec._original_control_layer_in_features == 16 and spec._original_control_layer_out_features == D
    assert spec._qk_norm_identifiers == ["norm_q", "norm_k", "norm_added_q", "norm_added_k"] and spec._resolution_dim_keys == {"latents": (2, 3, 4)}
    spec._trainer_init("index", 0, False)
    assert (spec.frame_conditioning_type, spec.frame_conditioning_index, spec.frame_conditioning_concatenate_mask) == ("index", 0, False)
    sd = {k: v.clone() for k, v in _model(1).state_dict_views().items()}
    out = spec.load_diffusion_models(32, state_dict=sd, device=torch.device("cpu"))
    assert out["transformer"].config.in_channels == 32 and spec._original_control_layer_in_features == 16  # the ORIGINAL width stays with the specification
    assert spec.transformer_config.num_layers == 1


def test_the_four_refusals():
    from finetrainers_amd.wan import MI355XWanControlModelSpecification, MI355XWanControlSpecOps, WanTransformerConfig

    spec = MI355XWanControlModelSpecification(pretrained_model_name_or_path=None)
    with pytest.raises(NotImplementedError, match="mask"):
        spec._trainer_init("full", 0, True)
    ops_ = MI355XWanControlSpecOps()
    ops_.frame_conditioning_concatenate_mask = True
    with pytest.raises(NotImplementedError, match="mask"):
        ops_.forward(lambda **kw: None, torch.zeros(1, 32, 1, 2, 2), torch.zeros(1, 4, 64), torch.tensor([0.5]), torch.zeros(16), torch.ones(16),
                     control_latents=torch.zeros(1, 32, 1, 2, 2))
    with pytest.raises(NotImplementedError, match="train_qk_norm"):
        spec.check_training_arguments("control-lora", train_qk_norm=True)
    with pytest.raises(NotImplementedError, match="control-full-finetune"):
        spec.check_training_arguments("control-full-finetune")
    spec.check_training_arguments("control-lora")
    i2v = MI355XWanControlModelSpecification(pretrained_model_name_or_path=None, transformer_config=WanTransformerConfig(num_layers=1, in_channels=36, image_dim=128, **SMALL))
    sd = {k: v.clone() for k, v in _model(1, in_channels=36, image_dim=128).state_dict_views().items()}
    with pytest.raises(NotImplementedError, match="image-to-video"):
        i2v.load_diffusion_models(72, state_dict=sd, device=torch.device("cpu"))


def test_c_abi_declares_exports_and_binds_the_control_symbols():
    from finetrainers_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in ("ftmi_f32_gemm", "ftmi_wan_control_pack", "ftmi_wan_patch_lora_forward", "ftmi_wan_patch_lora_backward"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
    # refusals that need no device: the checks run before any launch
    import ctypes

    for bad in (dict(r=96), dict(Kp=96), dict(D=96)):
        cfg = _lib.WanPatchLoraConfig(**dict(dict(M=18, D=256, Kp=128, r=256, s=1.0, gemm_variant=8, refold=0), **bad))
        one = ctypes.c_void_p(64)
        assert lib.ftmi_wan_patch_lora_forward(ctypes.byref(cfg), one, one, one, one, one, one, one, one, None) == _lib.FTMI_ERR_UNSUPPORTED, bad
        assert lib.ftmi_wan_patch_lora_backward(ctypes.byref(cfg), one, one, one, one, one, one, one, None) == _lib.FTMI_ERR_UNSUPPORTED, bad
    assert lib.ftmi_f32_gemm(64, 64, 96, ctypes.c_void_p(64), 96, 1, ctypes.c_void_p(64), 64, 1, ctypes.c_void_p(64), 64, 1.0, 0, None, 0, None) == _lib.FTMI_ERR_UNSUPPORTED


def test_the_gemm_launcher_accepts_the_folded_forward():
    """``ftmi_gemm_nt_route`` (host only): K = Kp = 128 with the K-extension K2 = 2 Kp runs as a tiled launch at both model widths and at the test widths."""
    from finetrainers_amd import ops

    for M, N in ((20280, 1536), (20280, 5120), (18, 256), (200, 384)):
        kind, _, bm, bn = ops.gemm_nt_route(M=M, N=N, K=128, K2=256, ldx=256, ldw=128, ldx2=256, ldw2=256, ldo=N)
        assert kind in (1, 2) and bm > 0 and bn > 0, (M, N, kind)
