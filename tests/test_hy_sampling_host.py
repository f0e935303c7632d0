"""HunyuanVideo latent sampling, the parts that need no GPU: the shifted flow-match sigmas against their closed form, the torch restatement
(tests/hy_sampling_reference.py: the loop the GPU trajectory test drives the oracle with), every refusal of the sampler with its reason, the argument checks
of the C entry points (they run before any launch), the workspace plan and the ABI table."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

import hy_sampling_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bf16 = torch.bfloat16
NEW_SYMBOLS = ("ftmi_hy_sample_init", "ftmi_hy_sample_step", "ftmi_hy_sample_finish", "ftmi_hy_sample_text_workspace_bytes", "ftmi_hy_sample_text")


# ---- the schedule ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 50])
@pytest.mark.parametrize("shift", [7.0, 1.0, 3.0, 17.0])
def test_sigmas_are_the_closed_form(n, shift):
    from finetrainers_amd.hunyuan_video import hy_flow_match_sigmas

    sig = hy_flow_match_sigmas(n, {"num_train_timesteps": 1000, "shift": shift})
    assert sig.dtype == torch.float64 and sig.shape == (n + 1,)
    closed = [shift * (1 - i / n) / (1 + (shift - 1) * (1 - i / n)) for i in range(n + 1)]
    assert max(abs(float(a) - b) for a, b in zip(sig, closed)) <= 1e-12
    assert float(sig[0]) == 1.0 and float(sig[n]) == 0.0
    assert bool((sig[1:] < sig[:-1]).all()), "strictly decreasing"
    assert float((sig - ref.sigmas(n, shift)).abs().max()) <= 1e-12, "the scheduler's own route: linspace, static shift, terminal zero"


def test_sigmas_defaults_and_refusals():
    from finetrainers_amd.hunyuan_video import HY_SCHEDULER_CONFIG, hy_flow_match_sigmas

    assert HY_SCHEDULER_CONFIG == {"num_train_timesteps": 1000, "shift": 7.0}
    assert torch.equal(hy_flow_match_sigmas(4), hy_flow_match_sigmas(4, dict(HY_SCHEDULER_CONFIG)))
    lin = hy_flow_match_sigmas(8, {"shift": 1.0})
    assert float((lin - torch.linspace(1, 0, 9, dtype=torch.float64)).abs().max()) <= 1e-15, "shift = 1 is linspace(1, 0, n + 1)"
    with pytest.raises(NotImplementedError, match="use_dynamic_shifting"):
        hy_flow_match_sigmas(4, {"shift": 7.0, "use_dynamic_shifting": True})
    with pytest.raises(ValueError, match="at least one step"):
        hy_flow_match_sigmas(0)
    with pytest.raises(ValueError, match="shift must be positive"):
        hy_flow_match_sigmas(4, {"shift": 0.0})


# ---- the torch restatement ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F_,H,W,pt", [(1, 2, 2, 1), (3, 4, 6, 1), (2, 4, 8, 2)])
def test_reference_layout_round_trips_and_orders_columns_as_the_patch_embedding(F_, H, W, pt):
    C, p = 4, 2
    lat = torch.arange(2 * C * F_ * H * W, dtype=torch.float32).reshape(2, C, F_, H, W)
    tok = ref.patchify(lat, p, pt)
    assert tok.shape == (2, (F_ // pt) * (H // p) * (W // p), C * pt * p * p)
    assert torch.equal(ref.unpatchify(tok, C, F_, H, W, p, pt), lat)
    # token (f', h', w'), column ((c pt + dt) p + dy) p + dx is latents[b, c, f' pt + dt, h' p + dy, w' p + dx]
    hpn, wpn = H // p, W // p
    for (b, t, k) in [(0, 0, 0), (1, tok.shape[1] - 1, tok.shape[2] - 1), (1, tok.shape[1] // 2, 5)]:
        fp, hp, wp = t // (hpn * wpn), (t // wpn) % hpn, t % wpn
        c, dt, dy, dx = k // (pt * p * p), (k // (p * p)) % pt, (k // p) % p, k % p
        assert float(tok[b, t, k]) == float(lat[b, c, fp * pt + dt, hp * p + dy, wp * p + dx])


def test_reference_trajectory_with_a_linear_model_is_the_product_of_the_step_maps():
    """v = a x: x_n = x_0 prod(1 + a (sigma_{i+1} - sigma_i)); with true CFG over u = a_u x, c = a_c x the effective slope is a_u + g (a_c - a_u)."""
    sig = ref.sigmas(6)
    x0 = torch.randn(2, 5, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    a = -0.7
    seen = []
    out = ref.trajectory(lambda x, i, t: (seen.append((i, t)), a * x)[1], x0, sig)
    prod = 1.0
    for i in range(6):
        prod *= 1.0 + a * (float(sig[i + 1]) - float(sig[i]))
    assert float((out - prod * x0).abs().max()) <= 1e-14
    assert [i for i, _ in seen] == list(range(6)) and seen[0][1] == 1000.0 and all(abs(t - 1000 * float(sig[i])) < 1e-9 for i, t in seen)
    au, ac, g = 0.3, -0.9, 3.0
    out = ref.trajectory(lambda x, i, t: torch.cat([au * x, ac * x]), x0, sig, true_cfg=g)
    prod = 1.0
    for i in range(6):
        prod *= 1.0 + (au + g * (ac - au)) * (float(sig[i + 1]) - float(sig[i]))
    assert float((out - prod * x0).abs().max()) <= 1e-13
    rounded = ref.trajectory(lambda x, i, t: a * x, x0.float(), sig, round_to=bf16)
    assert torch.equal(rounded, rounded.to(bf16).float()) and not torch.equal(rounded, (prod * x0).float())


# ---- what the sampler refuses ----------------------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from finetrainers_amd.hunyuan_video import HunyuanVideoTransformerConfig, MI355XHunyuanVideoTransformer3DModel

    cfg = dict(num_attention_heads=2, num_layers=1, num_single_layers=1, num_refiner_layers=1, text_embed_dim=64, pooled_projection_dim=64)
    cfg.update(kw)
    return MI355XHunyuanVideoTransformer3DModel(HunyuanVideoTransformerConfig(**cfg), device=torch.device("cpu"))


def _inputs(B=1, T=8):
    return torch.zeros(B, T, 64, dtype=bf16), torch.ones(B, T, dtype=torch.bool), torch.zeros(B, 64, dtype=bf16)


def test_sampler_refusals_name_their_reason():
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoLatentSampler

    noise = torch.zeros(1, 16, 3, 8, 12)
    e, m, p = _inputs()
    s = MI355XHunyuanVideoLatentSampler(_model())
    with pytest.raises(ValueError, match="true_cfg_scale != 1 needs negative_prompt_embeds"):
        s.sample(noise, e, m, p, true_cfg_scale=3.0)
    with pytest.raises(ValueError, match="true_cfg_scale != 1 needs negative_prompt_embeds"):
        s.sample(noise, e, m, p, negative_prompt_embeds=e, true_cfg_scale=3.0)
    with pytest.raises(ValueError, match="shaped like the prompt's"):
        s.sample(noise, e, m, p, negative_prompt_embeds=_inputs(B=2)[0], negative_pooled_prompt_embeds=p, true_cfg_scale=3.0)
    with pytest.raises(ValueError, match="prompt_embeds must be"):
        s.sample(noise, torch.zeros(1, 8, 32), m, p)
    with pytest.raises(ValueError, match="pooled_prompt_embeds must be"):
        s.sample(noise, e, m, torch.zeros(1, 32))
    with pytest.raises(ValueError, match="prompt_attention_mask must be"):
        s.sample(noise, e, torch.ones(1, 7), p)
    with pytest.raises(RuntimeError, match="load_diffusers_state_dict first"):
        s.sample(noise, e, m, p)
    with pytest.raises(NotImplementedError, match="guidance_embeds = False"):
        MI355XHunyuanVideoLatentSampler(_model(guidance_embeds=False)).sample(noise, e, m, p)
    with pytest.raises(NotImplementedError, match="patch_size_t = 2"):
        MI355XHunyuanVideoLatentSampler(_model(patch_size_t=2)).sample(noise, e, m, p)
    # past the model checks: a stand-in that claims to be loaded
    tr = _model()
    loaded = SimpleNamespace(config=tr.config, proj_out_w_t=torch.zeros(1), device=torch.device("cpu"), transformer_blocks=tr.transformer_blocks,
                             single_transformer_blocks=tr.single_transformer_blocks)
    s = MI355XHunyuanVideoLatentSampler(loaded)
    with pytest.raises(ValueError, match="latents must be"):
        s.sample(torch.zeros(1, 8, 3, 8, 12), e, m, p)
    with pytest.raises(ValueError, match="latents must be"):
        s.sample(torch.zeros(2, 16, 3, 8, 12), e, m, p)
    with pytest.raises(ValueError, match="multiples of patch_size"):
        s.sample(torch.zeros(1, 16, 3, 7, 12), e, m, p)
    with pytest.raises(ValueError, match="multiples of patch_size"):
        s.sample(torch.zeros(1, 16, 3, 8, 13), e, m, p)
    with pytest.raises(NotImplementedError, match="use_dynamic_shifting"):
        MI355XHunyuanVideoLatentSampler(loaded, {"shift": 7.0, "use_dynamic_shifting": True}).sample(noise, e, m, p)


def test_specification_gains_validation_latents_and_keeps_the_inherited_validation():
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoModelSpecification

    cls = MI355XHunyuanVideoModelSpecification
    assert callable(getattr(cls, "validation_latents"))
    assert all("validation" not in vars(b) for b in cls.__mro__ if b.__module__.startswith("finetrainers_amd.hunyuan_video"))
    spec = cls(pretrained_model_name_or_path=None)
    e, m, p = _inputs()
    with pytest.raises(ValueError, match="true_cfg_scale != 1 needs negative_prompt_embeds"):
        spec.validation_latents(_model(), e, m, p, 3, 8, 12, true_cfg_scale=2.0, latents=torch.zeros(1, 16, 3, 8, 12))
    with pytest.raises(RuntimeError, match="load_diffusers_state_dict first"):  # the noise is drawn, the inputs pass, the unloaded model does not
        spec.validation_latents(_model(), e, m, p, 3, 8, 12, generator=torch.Generator().manual_seed(0))


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------------------------------
def _geo(**kw):
    from finetrainers_amd import _lib

    base = dict(B=1, C=16, F=3, H=8, W=12, p=2, pt=1, P=1)
    base.update(kw)
    return _lib.HySampleGeometry(**base)


def test_c_abi_declares_exports_and_binds_the_sampling_symbols():
    from finetrainers_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
    import hy_sample_bytes

    hy_sample_bytes.assert_only_the_text_entries(lib, declared, set(_lib.EXPORTED_SYMBOLS))  # the pair over the bare ftmi_hy_sample_config is gone
    assert ctypes.sizeof(_lib.HySampleGeometry) == 32 and ctypes.sizeof(_lib.HySampleUpcast) == 24
    assert ctypes.sizeof(_lib.HySampleConfig) == 32 + 12 * 4 and ctypes.sizeof(_lib.HySampleWeights) == 11 * 8


def test_layout_kernels_check_their_arguments_before_any_launch():
    from finetrainers_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(256)
    step = lambda geo, pred=p, x=p, cols=p, g=1.0, sig=p, i=0: lib.ftmi_hy_sample_step(ctypes.byref(geo), pred, x, sig, i, g, cols, None)
    bad = [(dict(C=15), _lib.FTMI_ERR_UNSUPPORTED, "multiple of 8"), (dict(W=13), _lib.FTMI_ERR_UNSUPPORTED, "whole patches"),
           (dict(H=7), _lib.FTMI_ERR_UNSUPPORTED, "whole patches"), (dict(pt=2, F=3), _lib.FTMI_ERR_UNSUPPORTED, "whole patches"),
           (dict(P=3), _lib.FTMI_ERR_INVALID, "P is 2"), (dict(P=0), _lib.FTMI_ERR_INVALID, "P is 2"), (dict(B=0), _lib.FTMI_ERR_INVALID, "positive"),
           (dict(F=0), _lib.FTMI_ERR_INVALID, "positive"), (dict(p=0), _lib.FTMI_ERR_INVALID, "positive")]
    for kw, code, msg in bad:
        assert step(_geo(**kw)) == code and msg in _lib.last_error(), (kw, _lib.last_error())
    assert step(_geo(), pred=ctypes.c_void_p(264)) == _lib.FTMI_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert step(_geo(), x=ctypes.c_void_p(260)) == _lib.FTMI_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert step(_geo(), cols=ctypes.c_void_p(258)) == _lib.FTMI_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert step(_geo(), g=3.0) == _lib.FTMI_ERR_INVALID and "true_cfg" in _lib.last_error()
    assert step(_geo(P=2), g=1.0) == _lib.FTMI_ERR_INVALID and "true_cfg" in _lib.last_error()
    assert step(_geo(), sig=None) == _lib.FTMI_ERR_INVALID and "sigma table" in _lib.last_error()
    assert step(_geo(), i=-1) == _lib.FTMI_ERR_INVALID and "sigma table" in _lib.last_error()
    assert step(_geo(), pred=None, cols=None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_hy_sample_init(ctypes.byref(_geo(W=13)), p, p, p, None) == _lib.FTMI_ERR_UNSUPPORTED
    assert lib.ftmi_hy_sample_init(ctypes.byref(_geo()), p, p, ctypes.c_void_p(258), None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_hy_sample_init(ctypes.byref(_geo()), None, p, p, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_hy_sample_finish(ctypes.byref(_geo(C=15)), p, 1.0, p, None) == _lib.FTMI_ERR_UNSUPPORTED
    assert lib.ftmi_hy_sample_finish(ctypes.byref(_geo()), None, 1.0, p, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_hy_sample_finish(ctypes.byref(_geo()), p, 1.0, ctypes.c_void_p(264), None) == _lib.FTMI_ERR_INVALID


def _cfg(Ld=2, Ls=3, true_cfg=1.0, **kw):
    """The small model of tests/test_gpu_hunyuan.py on the (3, 8, 12) grid: 72 video tokens, 8 text tokens (as the C entries take it: text_adapters = 0)."""
    from finetrainers_amd import _lib

    base = dict(geo=_geo(P=2 if true_cfg != 1.0 else 1), T=8, D=256, H=2, mlp=1024, Ld=Ld, Ls=Ls, r=64, lora_scale=1.0, eps=1e-6, gemm_variant=8, steps=4,
                true_cfg=true_cfg)
    base.update(kw)
    return _lib.HySampleTextConfig(base=_lib.HySampleConfig(**base), text_adapters=0)


def _training_saved_bytes(Ld, Ls, B=1):
    """What training keeps at the same shape: one `saved` area per dual block and sample, one per single block."""
    from finetrainers_amd import _lib

    lib = _lib.load()
    dual = _lib.HyDualConfig(T=8, S=72, D=256, H=2, mlp=1024, r=64, lora_scale=1.0, eps=1e-6, gemm_variant=8)
    single = _lib.HySingleConfig(B=B, T=8, S=72, D=256, H=2, mlp=1024, r=64, lora_scale=1.0, eps=1e-6, gemm_variant=8)
    return Ld * B * lib.ftmi_hy_dual_saved_bytes(ctypes.byref(dual)) + Ls * lib.ftmi_hy_single_saved_bytes(ctypes.byref(single))


def test_workspace_plan_is_forward_only():
    """Nothing in the plan grows with Ld or Ls: (1, 1) and (20, 40) plan the same bytes.  At the small geometry (B = 1, no true CFG, r = 64) the plan holds
    the six stream / joint buffers, one `saved` slot, one scratch area, the head's rows and pred (2 246 144 bytes); a dual block keeps 615 168 bytes per sample in training and a
    single block 546 560, so the `saved` areas of training pass the plan from 4 blocks on when both kinds are present and from 5 blocks on in any split
    ((0, 4) keeps 2 186 240, still below it)."""
    from finetrainers_amd import _lib

    lib = _lib.load()
    ws = lambda **kw: lib.ftmi_hy_sample_text_workspace_bytes(ctypes.byref(_cfg(**kw)))
    assert ws(Ld=1, Ls=1) > 0 and ws(Ld=1, Ls=1) == ws(Ld=20, Ls=40) == ws(Ld=2, Ls=3) == ws(Ld=0, Ls=1) == ws(Ld=1, Ls=0)
    for Ld, Ls in ((1, 1), (1, 2), (2, 1), (0, 4)):
        assert ws() >= _training_saved_bytes(Ld, Ls), "fewer blocks keep less than the plan"
    for Ld, Ls in ((1, 3), (2, 2), (3, 1), (4, 0), (0, 5), (5, 0), (2, 3), (20, 40)):
        assert ws(Ld=Ld, Ls=Ls) < _training_saved_bytes(Ld, Ls), (Ld, Ls, ws(Ld=Ld, Ls=Ls), _training_saved_bytes(Ld, Ls))
    assert ws(Ld=20, Ls=40) < _training_saved_bytes(20, 40) // 8
    assert ws(true_cfg=1.0) < ws(true_cfg=3.0)
    assert ws(steps=50) == ws(steps=4), "nothing is kept per step"
    assert 0 < ws(r=0) < ws()
    # refused configurations plan 0 bytes, with the reason in ftmi_last_error
    for kw, msg in ((dict(r=32), "LoRA rank"), (dict(steps=0), "positive"), (dict(T=0), "positive"), (dict(geo=_geo(P=2)), "P is 2"), (dict(H=3), "heads x 128"),
                    (dict(geo=_geo(C=8)), "multiple of 64"), (dict(geo=_geo(W=13)), "whole patches"), (dict(mlp=1000), "multiple of 128"),
                    (dict(Ld=0, Ls=0), "at least one block"), (dict(Ld=-1), "at least one block")):
        assert ws(**kw) == 0 and msg in _lib.last_error(), (kw, _lib.last_error())


def test_sample_refuses_a_small_workspace_and_missing_weights():
    from finetrainers_amd import _lib

    lib = _lib.load()
    cfg = _cfg()
    need = lib.ftmi_hy_sample_text_workspace_bytes(ctypes.byref(cfg))
    p = ctypes.c_void_p(256)
    w = _lib.HySampleWeights()
    call = lambda nbytes, ws=p, w=w: lib.ftmi_hy_sample_text(ctypes.byref(cfg), ctypes.byref(w), p, p, p, p, p, p, None, p, p, p, ws, nbytes, None)
    assert call(need - 1) == _lib.FTMI_ERR_INVALID and "workspace too small" in _lib.last_error()
    assert call(need, ctypes.c_void_p(264)) == _lib.FTMI_ERR_INVALID and "256-byte aligned" in _lib.last_error()
    assert call(need) == _lib.FTMI_ERR_INVALID and "weights missing" in _lib.last_error()
    for f in ("patch_w", "patch_b", "proj_w", "proj_b", "ones", "zeros"):
        setattr(w, f, 256)
    assert call(need) == _lib.FTMI_ERR_INVALID and "weights missing" in _lib.last_error()  # the block arrays
    dual, single = (_lib.HyDualWeights * 2)(), (_lib.HySingleWeights * 3)()
    w.dual, w.single = ctypes.cast(dual, ctypes.POINTER(_lib.HyDualWeights)), ctypes.cast(single, ctypes.POINTER(_lib.HySingleWeights))
    ups = (_lib.HySampleUpcast * 1)()
    w.upcasts = ctypes.cast(ups, ctypes.POINTER(_lib.HySampleUpcast))
    assert call(need) == _lib.FTMI_ERR_INVALID and "counts and the arena" in _lib.last_error()
    assert lib.ftmi_hy_sample_text(ctypes.byref(cfg), ctypes.byref(w), None, p, p, p, p, p, None, p, p, p, p, need, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_hy_sample_text(ctypes.byref(cfg), ctypes.byref(w), p, p, p, p, p, p, None, p, p, None, p, need, None) == _lib.FTMI_ERR_INVALID
