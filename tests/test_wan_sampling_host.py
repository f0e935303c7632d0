"""Wan latent sampling, the parts that need no GPU: the sigma table against the scheduler's closed form, the torch restatement of the layout kernels
(tests/wan_sampling_reference.py: the loop the GPU trajectory test drives the oracle with), every refusal of the sampler with its message, the argument
checks of the C entry points (they run before any launch) and the ABI table."""
import ctypes
import os
import re

import pytest
import torch

import wan_sampling_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ref.SMALL
bf16 = torch.bfloat16
NEW_SYMBOLS = ("ftmi_wan_sample_init", "ftmi_wan_sample_step", "ftmi_wan_sample_finish", "ftmi_wan_sample_mod", "ftmi_wan_sample_workspace_bytes", "ftmi_wan_sample")


def _model(layers=1, **kw):
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig

    return MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, **SMALL, **kw), device=torch.device("cpu"))


# ---- the schedule --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 50])
def test_sigmas_at_shift_1_are_the_linear_table(n):
    from finetrainers_amd.wan import wan_flow_match_sigmas

    s = wan_flow_match_sigmas(n)
    assert s.dtype == torch.float32 and s.shape == (n + 1,) and float(s[-1]) == 0.0 and float(s[0]) == 1.0
    assert bool((s[1:] < s[:-1]).all())
    assert torch.equal(s[:-1], torch.linspace(1.0, 1.0 / 1000, n, dtype=torch.float64).float())
    assert torch.equal(s, wan_flow_match_sigmas(n, {"num_train_timesteps": 1000, "shift": 1.0}))


@pytest.mark.parametrize("n", [3, 20])
def test_sigmas_at_shift_3_follow_the_closed_form(n):
    """The scheduler shifts twice: sigma_min is the shifted 1 / N (sigma_max stays 1), and the linear table between them is shifted again:
    sigma_i = 3 l_i / (1 + 2 l_i), l_i = 1 + (sigma_min - 1) i / (n - 1), sigma_min = (3 / N) / (1 + 2 / N)."""
    from finetrainers_amd.wan import wan_flow_match_sigmas

    N, shift = 1000.0, 3.0
    s = wan_flow_match_sigmas(n, {"num_train_timesteps": 1000, "shift": shift}).double()
    smin = (shift / N) / (1 + (shift - 1) / N)
    want = [shift * l / (1 + (shift - 1) * l) for l in (1 + (smin - 1) * i / (n - 1) for i in range(n))]
    assert float(s[0]) == 1.0 and float(s[-1]) == 0.0 and bool((s[1:] < s[:-1]).all())
    assert torch.allclose(s[:-1], torch.tensor(want, dtype=torch.float64), rtol=0, atol=2.0 ** -24)  # one fp32 rounding of values <= 1
    assert abs(float(s[-2]) - shift * smin / (1 + (shift - 1) * smin)) < 2.0 ** -24


def test_sigmas_refuse_what_the_reference_does_not_build():
    from finetrainers_amd.wan import wan_flow_match_sigmas

    with pytest.raises(ValueError, match="at least one step"):
        wan_flow_match_sigmas(0)
    with pytest.raises(NotImplementedError, match="dynamic shifting"):
        wan_flow_match_sigmas(4, {"use_dynamic_shifting": True})


# ---- the torch restatement -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F_,H,W", [(1, 2, 2), (3, 4, 6)])
def test_reference_init_and_finish_round_trip_exactly(F_, H, W):
    g = torch.Generator().manual_seed(F_ + W)
    lat = torch.randn(2, 16, F_, H, W, generator=g)
    extra = torch.randn(2, 20, F_, H, W, generator=g).to(bf16)
    x, cols = ref.init_ref(lat, extra, Kp=192, copies=1, P=2)
    S = F_ * (H // 2) * (W // 2)
    assert x.shape == (2, S, 64) and cols.shape == (2 * 2 * S, 192)
    assert torch.equal(ref.unpatchify(x, 16, F_, H, W), lat), "x holds the latents' values exactly"
    assert torch.equal(cols[:2 * S], cols[2 * S:]) and torch.equal(cols[:, :64].float(), x.reshape(-1, 64).to(bf16).float().repeat(2, 1))
    assert torch.equal(ref.unpatchify(cols[:2 * S, 64:144].reshape(2, S, 80), 20, F_, H, W), extra)
    assert float(cols[:, 144:].float().abs().max()) == 0.0 and not bool(torch.signbit(cols[:, 144:].float()).any())
    back = ref.finish_ref(x, torch.zeros(16), torch.ones(16), 16, F_, H, W).to(bf16)
    assert torch.equal(back, lat.to(bf16))
    # column order: channel c, then (pt, ph, pw)
    assert float(x[0, 0, 5]) == float(lat[0, 1, 0, 0, 1]) and float(x[0, 0, 6]) == float(lat[0, 1, 0, 1, 0])


def test_reference_step_reads_pred_through_the_permutation():
    """pred column p C + c feeds state column c pv + p; guidance 1 takes the conditional rows as they are."""
    B, S, C, pv = 1, 3, 16, 4
    pred = (torch.arange(64).float() + 64 * torch.arange(S).float().view(S, 1)).view(1, S, 64).to(bf16)
    x = torch.zeros(B, S, 64)
    out = ref.step_ref(pred, x, torch.tensor([1.0]), torch.tensor([0.0]), 1.0, C)  # dt = -1
    for c in (0, 3, 15):
        for p in range(pv):
            assert float(out[0, 2, c * pv + p]) == -(p * C + c + 64 * 2)
    both = torch.cat([pred, 2 * pred.float()]).to(bf16)
    out = ref.step_ref(both, x, torch.tensor([0.5]), torch.tensor([0.25]), 5.0, C)
    assert torch.equal(out, -0.25 * (pred.double() + 5.0 * pred.double())[:, :, ref.pred_in_state_order(torch.arange(64).view(1, 1, 64), C).flatten()])


def test_reference_loop_moves_the_state_with_a_known_model():
    """A "model" that returns its input: with guidance g the combine is the identity, so x_n = x_0 prod (1 + sigma_{i+1} - sigma_i) up to the bf16 the model sees."""
    lat = torch.randn(1, 16, 1, 4, 4, generator=torch.Generator().manual_seed(0))
    fn = lambda hidden_states, timestep, encoder_hidden_states, return_dict: (hidden_states,)
    text = torch.zeros(1, 2, 8)
    x = ref.trajectory(fn, torch.float32, lat, text, text, [1.0, 0.5, 0.0], 5.0)
    assert torch.allclose(x, ref.patchify(lat) * 0.25, rtol=1e-6, atol=0)


# ---- what the sampler refuses ----------------------------------------------------------------------------------------------------------------------------------
def _embeds(B=1, T=16):
    return torch.zeros(B, T, 64, dtype=bf16)


def test_sampler_refusals_name_their_reason():
    from finetrainers_amd.wan import MI355XWanLatentSampler

    grid = dict(num_frames=2, height=8, width=12)
    t2v = MI355XWanLatentSampler(_model())
    with pytest.raises(ValueError, match="guidance_scale != 1 needs negative_prompt_embeds"):
        t2v.sample(_embeds(), None, **grid)
    with pytest.raises(ValueError, match="shaped like prompt_embeds"):
        t2v.sample(_embeds(), _embeds(T=8), **grid)
    with pytest.raises(ValueError, match="image-to-video model"):
        t2v.sample(_embeds(), _embeds(), image_embeds=torch.zeros(1, 5, 64), **grid)
    with pytest.raises(ValueError, match="image-to-video model"):
        t2v.sample(_embeds(), _embeds(), condition_latents=torch.zeros(1, 20, 2, 8, 12), **grid)
    with pytest.raises(ValueError, match="patch embedding was widened"):
        t2v.sample(_embeds(), _embeds(), control_latents=torch.zeros(1, 16, 2, 8, 12), **grid)
    with pytest.raises(ValueError, match="prompt_embeds must be"):
        t2v.sample(torch.zeros(1, 16, 32), None, guidance_scale=1.0, **grid)
    with pytest.raises(ValueError, match="latents must be"):
        t2v.sample(_embeds(), _embeds(), latents=torch.zeros(1, 16, 2, 8, 10), **grid)
    with pytest.raises(ValueError, match="one value per step"):
        t2v.sample(_embeds(), _embeds(), sigmas=[1.0, 0.5, 0.0], timesteps=[1000.0], **grid)

    i2v = MI355XWanLatentSampler(_model(image_dim=64, in_channels=36))
    assert i2v.extra_channels == 20
    with pytest.raises(ValueError, match="needs image_embeds and condition_latents"):
        i2v.sample(_embeds(), _embeds(), **grid)
    with pytest.raises(ValueError, match="needs image_embeds and condition_latents"):
        i2v.sample(_embeds(), _embeds(), image_embeds=torch.zeros(1, 5, 64), **grid)
    with pytest.raises(ValueError, match="condition_latents must be"):
        i2v.sample(_embeds(), _embeds(), image_embeds=torch.zeros(1, 5, 64), condition_latents=torch.zeros(1, 16, 2, 8, 12), **grid)
    with pytest.raises(ValueError, match="image_embeds must be"):
        i2v.sample(_embeds(), _embeds(), image_embeds=torch.zeros(1, 5, 32), condition_latents=torch.zeros(1, 20, 2, 8, 12), **grid)

    widened = _model()
    widened.expand_patch_embedding(32)
    control = MI355XWanLatentSampler(widened)
    assert control.extra_channels == 16
    with pytest.raises(ValueError, match="needs control_latents"):
        control.sample(_embeds(), _embeds(), **grid)
    with pytest.raises(ValueError, match="control_latents must be"):
        control.sample(_embeds(), _embeds(), control_latents=torch.zeros(1, 16, 3, 8, 12), **grid)

    sharded = _model()
    sharded.root = torch.nn.Parameter(sharded.root.data[:128].clone(), requires_grad=False)
    with pytest.raises(RuntimeError, match="sharded over the ranks"):
        MI355XWanLatentSampler(sharded).sample(_embeds(), _embeds(), **grid)


def test_specifications_gain_validation_latents_and_keep_the_inherited_validation():
    from finetrainers_amd.wan import MI355XWanControlModelSpecification, MI355XWanModelSpecification

    for cls in (MI355XWanModelSpecification, MI355XWanControlModelSpecification):
        assert callable(getattr(cls, "validation_latents"))
        assert "validation" not in cls.__dict__ and all("validation" not in vars(b) for b in cls.__mro__ if b.__module__.startswith("finetrainers_amd.wan"))
    spec = MI355XWanModelSpecification(pretrained_model_name_or_path=None)
    with pytest.raises(ValueError, match="guidance_scale != 1 needs negative_prompt_embeds"):
        spec.validation_latents(_model(), _embeds(), None, 2, 8, 12)
    cspec = MI355XWanControlModelSpecification(pretrained_model_name_or_path=None)
    with pytest.raises(ValueError, match="patch embedding was widened"):  # the control latents are normalised and frame-conditioned, then the sampler refuses the model
        cspec.validation_latents(_model(), _embeds(), _embeds(), torch.zeros(1, 16, 1, 8, 12), 2, 8, 12, torch.zeros(16), torch.ones(16))


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------------------------------
def _geo(**kw):
    from finetrainers_amd import _lib

    base = dict(B=1, C=16, Cx=0, F=2, H=8, W=12, pt=1, ph=2, pw=2, Kp=64, copies=1, P=2, po=64)
    base.update(kw)
    return _lib.WanSampleGeometry(**base)


def test_c_abi_declares_exports_and_binds_the_sampling_symbols():
    from finetrainers_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name


def test_layout_kernels_check_their_arguments_before_any_launch():
    from finetrainers_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(256)
    step = lambda geo, pred=p, x=p, cols=p, g=5.0: lib.ftmi_wan_sample_step(ctypes.byref(geo), pred, x, p, p, g, cols, None)
    bad = [(dict(C=15, po=60), _lib.FTMI_ERR_UNSUPPORTED, "multiples of 8"), (dict(Kp=68), _lib.FTMI_ERR_UNSUPPORTED, "row stride"),
           (dict(po=128), _lib.FTMI_ERR_INVALID, "must equal po"), (dict(W=13), _lib.FTMI_ERR_UNSUPPORTED, "whole patches"),
           (dict(H=7), _lib.FTMI_ERR_UNSUPPORTED, "whole patches"), (dict(pt=2, F=3), _lib.FTMI_ERR_UNSUPPORTED, "whole patches"),
           (dict(Cx=20), _lib.FTMI_ERR_INVALID, "do not fit"), (dict(copies=3), _lib.FTMI_ERR_INVALID, "copies"), (dict(P=3), _lib.FTMI_ERR_INVALID, "P is 2"),
           (dict(C=24, po=96, Kp=128), _lib.FTMI_ERR_UNSUPPORTED, "divide 2048")]
    for kw, code, msg in bad:
        assert step(_geo(**kw)) == code and msg in _lib.last_error(), (kw, _lib.last_error())
    assert step(_geo(), pred=ctypes.c_void_p(264)) == _lib.FTMI_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert step(_geo(), x=ctypes.c_void_p(260)) == _lib.FTMI_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert step(_geo(), g=1.0) == _lib.FTMI_ERR_INVALID and "guidance" in _lib.last_error()
    assert step(_geo(), pred=None, cols=None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_wan_sample_init(ctypes.byref(_geo(W=13)), p, None, p, p, None) == _lib.FTMI_ERR_UNSUPPORTED
    assert lib.ftmi_wan_sample_init(ctypes.byref(_geo(Cx=20, Kp=192)), p, None, p, p, None) == _lib.FTMI_ERR_INVALID and "extra channels" in _lib.last_error()
    assert lib.ftmi_wan_sample_init(ctypes.byref(_geo()), p, None, p, ctypes.c_void_p(258), None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_wan_sample_finish(ctypes.byref(_geo(po=32)), p, p, p, p, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_wan_sample_finish(ctypes.byref(_geo()), None, p, p, p, None) == _lib.FTMI_ERR_INVALID
    tables = (ctypes.c_void_p * 2)(256, 512)
    assert lib.ftmi_wan_sample_mod(tables, 2, p, p, 2, 2, None) == _lib.FTMI_ERR_UNSUPPORTED  # 6 D = 12 is no whole number of 16-byte vectors
    assert lib.ftmi_wan_sample_mod(tables, 41, p, p, 2, 256, None) == _lib.FTMI_ERR_UNSUPPORTED
    assert lib.ftmi_wan_sample_mod((ctypes.c_void_p * 2)(256, 520), 2, p, p, 2, 256, None) == _lib.FTMI_ERR_INVALID


def _cfg(L=2, guidance=5.0, **kw):
    from finetrainers_amd import _lib

    base = dict(geo=_geo(P=2 if guidance != 1.0 else 1), T=16, TI=0, D=256, heads=2, ffn_dim=512, L=L, eps=1e-6, gemm_variant=8, r=64, lora_scale=1.0, ffn=0,
                patch_fold=0, patch_r=0, patch_scale=0.0, steps=3, guidance=guidance)
    base.update(kw)
    return _lib.WanSampleConfig(**base)


def test_workspace_plan_is_forward_only():
    """The plan does not depend on the number of blocks (every block writes the same ``saved`` slot), it is smaller than L blocks' saved activations already
    at L = 4, and the run without guidance (conditional rows only) needs less than the one with it."""
    from finetrainers_amd import _lib

    lib = _lib.load()
    ws = lambda **kw: lib.ftmi_wan_sample_workspace_bytes(ctypes.byref(_cfg(**kw)))
    assert ws(L=4) > 0 and ws(L=4) == ws(L=2) == ws(L=1) == ws(L=40)
    blk = _lib.WanLoraFfnBlockConfig(B=2, S=48, T=16, D=256, H=2, F=512, eps=1e-6, gemm_variant=8, r=64, lora_scale=1.0, TI=0, ffn=0)
    saved = lib.ftmi_wan_lora_ffn_block_saved_bytes(ctypes.byref(blk))
    assert saved > 0 and ws(L=4) < 4 * saved, (ws(L=4), saved)
    assert ws(guidance=1.0) < ws(guidance=5.0)
    assert ws(steps=50) == ws(steps=3), "nothing is kept per step"
    # refused configurations plan 0 bytes, with the reason in ftmi_last_error
    for kw, msg in ((dict(L=41), "1 .. 40 blocks"), (dict(r=32), "LoRA rank"), (dict(patch_fold=1), "[cols | cols]"), (dict(steps=0), "positive"),
                    (dict(geo=_geo(P=1)), "P is 2"), (dict(TI=400), "image context")):
        assert ws(**kw) == 0 and msg in _lib.last_error(), (kw, _lib.last_error())


def test_sample_refuses_a_small_workspace_and_missing_weights():
    from finetrainers_amd import _lib

    lib = _lib.load()
    cfg = _cfg()
    need = lib.ftmi_wan_sample_workspace_bytes(ctypes.byref(cfg))
    p = ctypes.c_void_p(256)
    blocks = (_lib.WanLoraFfnBlockWeights * 2)()
    w = _lib.WanSampleWeights()
    w.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.WanLoraFfnBlockWeights))
    w.patch_w = w.patch_b = w.proj_w = w.proj_b = 256
    call = lambda nbytes: lib.ftmi_wan_sample(ctypes.byref(cfg), ctypes.byref(w), p, p, p, p, p, p, None, p, p, p, p, nbytes, None)
    assert call(need - 1) == _lib.FTMI_ERR_INVALID and "workspace too small" in _lib.last_error()
    assert call(need) == _lib.FTMI_ERR_INVALID and "block without parameters" in _lib.last_error()
    assert lib.ftmi_wan_sample(ctypes.byref(cfg), ctypes.byref(w), None, p, p, p, p, p, None, p, p, p, p, need, None) == _lib.FTMI_ERR_INVALID
