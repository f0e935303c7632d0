"""Wan LoRA with adapters on the feed-forward projections, the parts that need no GPU: which adapter set a ``target_modules`` selects (peft's rule, cross-checked
against ``re.fullmatch`` over the diffusers module names written out here), the state-dict keys / shapes / padding, the adapter file round trip, the C ABI of
the new entry points and their byte plans."""
import ctypes
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# examples/training/control/wan/image_condition/train.sh --target_modules, as written: "ff.net" is f, f, any character, n, e, t -- Wan's module is "ffn.net"
RECIPE_LITERAL = "blocks.*(to_q|to_k|to_v|to_out.0|ff.net.0.proj|ff.net.2)"
TEN_REGEX = "blocks.*(to_q|to_k|to_v|to_out.0|ffn.net.0.proj|ffn.net.2)"
TEN_LIST = ["to_q", "to_k", "to_v", "to_out.0", "net.0.proj", "net.2"]
SMALL = dict(num_attention_heads=2, attention_head_dim=128, ffn_dim=512, text_dim=64)
D, F = 256, 512
NEW_SYMBOLS = ("ftmi_wan_lora_ffn_block_saved_bytes", "ftmi_wan_lora_ffn_block_scratch_bytes", "ftmi_wan_lora_ffn_block_forward", "ftmi_wan_lora_ffn_block_backward")


def _module_names(layers, i2v):
    """Every Conv3d / Linear module name of diffusers' WanTransformer3DModel (what peft could wrap), independent of the code under test."""
    ce = "condition_embedder."
    names = ["patch_embedding", ce + "time_embedder.linear_1", ce + "time_embedder.linear_2", ce + "time_proj", ce + "text_embedder.linear_1", ce + "text_embedder.linear_2"]
    if i2v:
        names += [ce + "image_embedder.ff.net.0.proj", ce + "image_embedder.ff.net.2"]
    for i in range(layers):
        for a in ("attn1", "attn2"):
            names += [f"blocks.{i}.{a}.{t}" for t in ("to_q", "to_k", "to_v", "to_out.0")]
        if i2v:
            names += [f"blocks.{i}.attn2.add_k_proj", f"blocks.{i}.attn2.add_v_proj"]
        names += [f"blocks.{i}.ffn.net.0.proj", f"blocks.{i}.ffn.net.2"]
    return names + ["proj_out"]


def _peft_select(target_modules, names):
    if isinstance(target_modules, str):
        return [n for n in names if re.fullmatch(target_modules, n)]
    return [n for n in names if any(n == t or n.endswith("." + t) for t in target_modules)]


def _model(layers=2, i2v=False):
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig

    kw = dict(image_dim=128, in_channels=36) if i2v else {}
    return MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, **SMALL, **kw), device=torch.device("cpu"))


def test_the_model_lists_the_diffusers_linear_modules():
    for i2v in (False, True):
        assert sorted(_model(3, i2v).linear_module_names()) == sorted(_module_names(3, i2v))


@pytest.mark.parametrize("target,i2v,per_block", [(RECIPE_LITERAL, False, 8), (RECIPE_LITERAL, True, 8), (TEN_REGEX, False, 10), (TEN_REGEX, True, 10),
                                                   (TEN_LIST, False, 10), (tuple(TEN_LIST), False, 10)])
def test_target_modules_select_what_peft_selects(target, i2v, per_block):
    layers = 3
    selected = _peft_select(target, _module_names(layers, i2v))
    assert len(selected) == per_block * layers and all(n.startswith("blocks.") for n in selected)  # the expectation itself, by peft's rule
    model = _model(layers, i2v)
    model.add_adapter(32, 16.0, target_modules=target)
    assert model.lora_config == {"r": 32, "lora_alpha": 16.0, "target_modules": target}  # the user's value, unchanged
    sd = model.lora_state_dict()
    assert set(sd) == {f"{n}.lora_{ab}.weight" for n in selected for ab in "AB"}
    assert all((blk.lora_ffn is not None) == (per_block == 10) for blk in model.blocks)
    assert len(model.lora_parameters()) == layers * (6 if per_block == 10 else 2)


@pytest.mark.parametrize("target,i2v,offender", [
    (TEN_LIST, True, "condition_embedder.image_embedder.ff.net.0.proj"),  # the list form also hits the image embedder's feed-forward
    ("blocks.0.*(to_q)", False, "blocks.0.attn1.to_k"),                    # a subset: the first covered module it leaves out
    ("blocks.0.*(to_q|to_k|to_v|to_out.0)", False, "blocks.1.attn1.to_q"),  # some blocks only
    ("blocks.*(to_q|to_k|to_v|to_out.0|ffn.net.2)", False, "blocks.0.ffn.net.0.proj"),
    ("patch_embedding|" + TEN_REGEX, False, "patch_embedding"),
    (TEN_LIST + ["proj_out"], False, "proj_out"),
    (".*(to_q|to_k|to_v|to_out.0|time_proj)", False, "condition_embedder.time_proj"),
    ("blocks.*(to_q|to_k|to_v|to_out.0|add_k_proj)", True, "blocks.0.attn2.add_k_proj"),
])
def test_any_other_selection_raises_naming_the_module(target, i2v, offender):
    names = _module_names(2, i2v)
    selected = set(_peft_select(target, names))
    ten = {n for n in names if re.fullmatch(TEN_REGEX, n)}
    eight = {n for n in names if re.fullmatch("blocks.*(to_q|to_k|to_v|to_out.0)", n)}
    assert selected not in (eight, ten) and (offender in selected - ten or offender in ten - selected)  # the case is what it claims to be
    model = _model(2, i2v)
    with pytest.raises(NotImplementedError, match=re.escape(offender) + r"(;|$)"):
        model.add_adapter(32, 32.0, target_modules=target)
    assert model.lora_config is None and model.blocks[0].lora_A is None and model.blocks[0].lora_ffn is None


def test_a_pattern_that_selects_nothing_raises():
    model = _model(1)
    assert _peft_select("ffn.*", _module_names(1, False)) == []  # fullmatch: every name starts with "blocks."
    with pytest.raises(NotImplementedError, match="selects no module"):
        model.add_adapter(32, 32.0, target_modules="ffn.*")


def test_state_dict_keys_shapes_initialisation_and_padding():
    model = _model(2)
    model.add_adapter(32, 32.0, target_modules=TEN_REGEX)
    sd = model.lora_state_dict()
    want = {"ffn.net.0.proj.lora_A.weight": (32, D), "ffn.net.0.proj.lora_B.weight": (F, 32), "ffn.net.2.lora_A.weight": (32, F), "ffn.net.2.lora_B.weight": (D, 32)}
    for i in range(2):
        for k, shape in want.items():
            v = sd[f"blocks.{i}.{k}"]
            assert tuple(v.shape) == shape and v.dtype == torch.float32, k
            if ".lora_B." in k:
                assert float(v.abs().max()) == 0.0  # peft's init: B = 0
            else:  # kaiming_uniform_(a = sqrt(5)): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), fan_in = the layer's input width -- F for ffn.net.2
                fan_in = shape[1]
                assert 0.9 / fan_in ** 0.5 < float(v.abs().max()) <= 1.0 / fan_in ** 0.5, k
    for blk in model.blocks:  # rank 32 inside storage padded to the kernels' 64-row groups; the padding is zero
        a1, b1, a2, b2 = blk.lora_ffn
        assert tuple(a1.shape) == (64, D) and tuple(b1.shape) == (F, 64) and tuple(a2.shape) == (64, F) and tuple(b2.shape) == (D, 64)
        assert all(p.requires_grad and p.dtype == torch.float32 for p in blk.lora_ffn)
        assert float(a1.data[32:].abs().max()) == 0.0 and float(a2.data[32:].abs().max()) == 0.0
    assert len(sd) == 2 * 20 and len(model.lora_parameters()) == 12


def _randomise(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for v in model.lora_state_dict().values():
            v.copy_(0.02 * torch.randn(v.shape, generator=g))


def test_state_dict_and_adapter_file_round_trip(tmp_path):
    from finetrainers_amd import wire

    model = _model(2)
    model.add_adapter(32, 16.0, target_modules=TEN_REGEX)
    _randomise(model, 3)
    want = {k: v.clone() for k, v in model.lora_state_dict().items()}
    wire.save_lora_weights(str(tmp_path), model.lora_state_dict(), wire.lora_config_metadata(32, 16.0, TEN_REGEX))
    sd, cfg = wire.load_lora_weights(str(tmp_path))
    assert cfg["r"] == 32 and cfg["lora_alpha"] == 16.0 and cfg["target_modules"] == TEN_REGEX and json.dumps(cfg)
    assert set(sd) == set(want)
    fresh = _model(2)
    fresh.add_adapter(cfg["r"], cfg["lora_alpha"], target_modules=cfg["target_modules"])
    fresh.load_lora_state_dict({k.replace(".lora_A.", ".lora_A.default."): v for k, v in sd.items()})  # peft's own key form loads too
    got = fresh.lora_state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    for blk in fresh.blocks:  # loading leaves the padding rows / columns zero
        a1, b1, a2, b2 = blk.lora_ffn
        assert float(a1.data[32:].abs().max()) == 0.0 and float(a2.data[32:].abs().max()) == 0.0
        assert float(b1.data[:, 32:].abs().max()) == 0.0 and float(b2.data[:, 32:].abs().max()) == 0.0
        assert float(b1.data[:, :32].abs().max()) > 0.0
    with pytest.raises(KeyError):  # a file of the eight-adapter set does not fit the ten-adapter model ...
        fresh.load_lora_state_dict({k: v for k, v in sd.items() if ".ffn." not in k})
    eight = _model(2)
    eight.add_adapter(32, 16.0)
    with pytest.raises(KeyError):  # ... nor the other way round
        eight.load_lora_state_dict(sd)
    with pytest.raises(ValueError):
        fresh.load_lora_state_dict({k: (v.t().contiguous() if k == "blocks.1.ffn.net.2.lora_A.weight" else v) for k, v in sd.items()})


def test_step_object_lays_out_every_adapter_and_its_gradient():
    """``MI355XWanLoRAStep``'s flat buffers (built on the CPU: no kernel runs at construction): every adapter Parameter is a view of ``flat``, every block's
    gradient views tile one contiguous span of ``gflat`` in the same order, the spans follow each other (the bucketed exchange relies on it)."""
    from finetrainers_amd.wan import MI355XWanLoRAStep

    model = _model(3)
    model.add_adapter(32, 32.0, target_modules=TEN_REGEX)
    _randomise(model, 5)
    before = {k: v.clone() for k, v in model.lora_state_dict().items()}
    step = MI355XWanLoRAStep(model)
    assert step.flat.numel() == sum(p.numel() for p in model.lora_parameters()) == 3 * (16 * 64 * D + 2 * 64 * (D + F))
    assert all(torch.equal(v, before[k]) for k, v in model.lora_state_dict().items())
    off = 0
    for blk in model.blocks:
        views = [blk._grad_a_view, blk._grad_b_view] + list(blk._grad_ffn_views)
        assert step._spans[id(blk)][0] == off
        for p, gv in zip(blk.lora_parameters(), views):
            assert gv.shape == p.shape and gv.data_ptr() == step.gflat.data_ptr() + 4 * off and p.data_ptr() == step.flat.data_ptr() + 4 * off
            off += p.numel()
        assert step._spans[id(blk)][1] == off
    step.gflat.fill_(1.0)
    assert all(float(v.min()) == 1.0 for v in model.lora_grad_state_dict().values()) and set(model.lora_grad_state_dict()) == set(before)


class _RecordingParallel:
    """Stands in for the data-parallel backend: records the slices the step object hands to the asynchronous all-reduce."""
    active, world_size, rank = True, 1, 0

    def __init__(self):
        self.slices = []

    def broadcast_(self, t, src=0):
        pass

    def all_reduce_mean_async(self, t):
        self.slices.append((t.data_ptr(), t.numel()))
        return None


def test_gradient_hook_buckets_cover_the_ten_adapter_blocks():
    """The overlapped exchange as the blocks' backward drives it (last block first, each reporting itself finished through ``_grad_hook``): with six
    Parameters per block the buckets are still whole blocks, contiguous, and cover the flat gradient exactly once."""
    from finetrainers_amd.wan import MI355XWanLoRAStep

    model = _model(5)
    model.add_adapter(32, 32.0, target_modules=TEN_REGEX)
    par = _RecordingParallel()
    step = MI355XWanLoRAStep(model, parallel=par, grad_bucket_blocks=2)
    per_block = 16 * 64 * D + 2 * 64 * (D + F)
    step._begin_exchange(True)
    for blk in reversed(model.blocks):
        blk._backward_done()
    step._finish_exchange()
    assert step.bucket_log == [(3 * per_block, 5 * per_block), (per_block, 3 * per_block), (0, per_block)]  # {4, 3}, {2, 1}, {0}
    assert par.slices == [(step.gflat.data_ptr() + 4 * lo, hi - lo) for lo, hi in step.bucket_log]
    assert all(blk._grad_hook is None for blk in model.blocks)


def test_c_abi_exports_and_declares_the_ffn_lora_block():
    """The new symbols are declared in the header, exported by the library and bound (tests/test_host.py's header-driven test then covers them as well), and each
    declaration's comment cites the reference site it stands for."""
    import wan_lora_bytes
    from finetrainers_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
    wan_lora_bytes.assert_only_the_wide_family(lib, declared, set(_lib.EXPORTED_SYMBOLS))  # ... and they are the only LoRA block entries left
    before =header[:header.index("} ftmi_wan_lora_ffn_block_config;")].rsplit("typedef struct", 1)[0]
    comment = before.rsplit("/*", 1)[1]
    assert "finetrainers/trainer/sft_trainer/trainer.py" in comment and "ffn.net.0.proj" in comment


def _cfg(**kw):
    from finetrainers_amd import _lib

    base = dict(B=1, S=20280, T=512, D=1536, H=12, F=8960, eps=1e-6, gemm_variant=8, r=64, lora_scale=1.0, TI=0, ffn=0)
    base.update(kw)
    return _lib.WanLoraFfnBlockConfig(**base)


def test_byte_plans_of_the_new_entry():
    """ffn = 0: the byte counts recorded in tests/golden/wan_lora_entry_bytes.txt, which the text-to-video and image-to-video entries of the time returned as
    well, to the byte.  ffn = 1: `saved` grows by exactly n3, act and the two down-projected rows (each rounded up to the planner's 256-byte granule),
    whatever TI, and lands on the recorded bytes."""
    import wan_lora_bytes
    from finetrainers_amd import _lib

    lib = _lib.load()
    plans = wan_lora_bytes.recorded()
    geom = (1, 20280, 512, 1536, 12, 8960)
    up = lambda n: (n + 255) // 256 * 256
    for r in (0, 64, 128):
        for TI in (0, 257):
            off = _cfg(r=r, TI=TI)
            saved0, scratch0 = lib.ftmi_wan_lora_ffn_block_saved_bytes(ctypes.byref(off)), lib.ftmi_wan_lora_ffn_block_scratch_bytes(ctypes.byref(off))
            assert (saved0, scratch0) == plans[geom + (r, TI, 0)] and saved0 > 0 and scratch0 > 0
            if r:
                on = _cfg(r=r, TI=TI, ffn=1)
                M = 20280
                grow = up(M * 1536 * 2) + up(M * 8960 * 2) + 2 * up(M * 3 * r * 2)
                assert lib.ftmi_wan_lora_ffn_block_saved_bytes(ctypes.byref(on)) == saved0 + grow == plans[geom + (r, TI, 1)][0]
                assert lib.ftmi_wan_lora_ffn_block_scratch_bytes(ctypes.byref(on)) == plans[geom + (r, TI, 1)][1] > 0


@pytest.mark.parametrize("kw,code,word", [(dict(ffn=1, r=0), "UNSUPPORTED", "rank"), (dict(ffn=1, F=192), "UNSUPPORTED", "feed-forward width"),
                                          (dict(ffn=1, r=96), "UNSUPPORTED", "rank"), (dict(ffn=1, TI=400), "UNSUPPORTED", "image"), (dict(ffn=2), "INVALID", "ffn")])
def test_geometries_the_kernels_cannot_take_are_refused(kw, code, word):
    """A refused configuration plans 0 bytes and says why; the forward returns the error code before it touches a pointer."""
    from finetrainers_amd import _lib

    lib = _lib.load()
    cfg = _cfg(S=64, T=16, D=256, H=2, **{"F": 512, **kw})
    assert lib.ftmi_wan_lora_ffn_block_saved_bytes(ctypes.byref(cfg)) == 0 and word in _lib.last_error()
    assert lib.ftmi_wan_lora_ffn_block_scratch_bytes(ctypes.byref(cfg)) == 0
    w = _lib.WanLoraFfnBlockWeights()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    w.base.params = p
    rc = lib.ftmi_wan_lora_ffn_block_forward(ctypes.byref(cfg), ctypes.byref(w), p, p, p, p, p, p, p, p, p, 64, p, 64, None)
    assert rc == getattr(_lib, "FTMI_ERR_" + code) and word in _lib.last_error()
